"""LocalMapping's culling restated in plain Python from the reference's lines
(LocalMapping::MapPointCulling LocalMapping.cc:170-205 and KeyFrameCulling :632-698;
MapPoint::AddObservation / EraseObservation / SetBadFlag MapPoint.cc:339-409; GetFoundRatio;
KeyFrame::SetBadFlag / SetErase KeyFrame.cc:1158-1287; TrackedMapPoints KeyFrame.cc:971-996) over
the scripted map model of tests/covis_cases.py, with branch counters and single-decision
mutants; the built cases that tests/test_culling.py proves non-trivial and
tests/test_gpu_culling.py runs against the library; and the driver that replays a script on a
``native.LocalMap``.

The script operations of covis_cases are kept ("obs" / "unobs" are the index-less calls: index
unknown, nObs changes by 1).  New:
    ("features", kf, octaves|None, mvu_right|None, depth|None, th_depth)    answers what the getter
                                            reads back (depths as float32 bit patterns), no state
    ("obsidx", [(point, kf, idx), ...])     MapPoint::AddObservation(pKF, idx)
    ("eraseobs", point, kf)                 MapPoint::EraseObservation(pKF), with `nObs <= 2`
    ("counters", [points], nobs|None, found|None, visible|None, first|None)   plain assignment
    ("inc", "found"|"visible", [points], [amounts]|None)    IncreaseFound / IncreaseVisible
    ("mpbadflag", [points])                 MapPoint::SetBadFlag, complete
    ("cullpoints", [points], current_kf_id, monocular)      MapPointCulling
    ("tracked", kf, min_obs)                TrackedMapPoints
    ("noterase", kf, flag)                  mbNotErase
    ("kfbadflag", kf[, is_first])           KeyFrame::SetBadFlag, complete -> (what, points that
                                            went bad, (child, new parent) pairs)
    ("seterase", kf, has_loop_edges[, is_first])   KeyFrame::SetErase -> the same
    ("cullkfs", current, [kfs]|None, first|None, monocular)   KeyFrameCulling over the list, or over
                                            the current keyframe's ordered covisibility list ->
                                            (list, results, points that went bad, pairs)
The answer of each of them is the operation's own output and the whole state afterwards (every
keyframe's mvpMapPoints, bad, not-erase and to-be-erased flags; every point's bad flag, observation
row with indices, nObs, found, visible, first id; the graph and the spanning tree of every
keyframe); an operation the library refuses answers ("error", state) or ("capacity", state).
"""
from __future__ import annotations

import random

import numpy as np

import covis_cases as K
from localmap_cases import BASE, _bump, keys_for

MUTANTS = ("add_overwrites", "right_ignored", "erase_right_ignored", "bad_lt2", "erase_never_bad",
           "badflag_resets_nobs", "badflag_keeps_obs", "match_checked", "ratio_le", "ratio_double",
           "th_obs_2", "nobs_lt", "diff_gt", "branch_order", "old_kept", "dup_independent",
           "bad_listed_kept", "tracked_counts_bad", "tracked_gt", "tracked_ignores_obs",
           # KeyFrame::SetBadFlag, SetErase, KeyFrameCulling
           "one_shot", "cull_ge", "kf_th_obs_2", "octave_plus_0", "self_counted", "depth_in_mono",
           "depth_ge", "right_at_i", "kf_bad_lt2", "tournament_ordered_weights", "tournament_ge",
           "bad_child_reassigned", "children_cleared", "conn_after_tree", "noterase_ignored",
           "first_culled", "seterase_keeps_flag", "held_twice_counts_once", "bad_point_in_nmps")

OPS = ("features", "obsidx", "eraseobs", "counters", "inc", "mpbadflag", "cullpoints", "tracked",
       "noterase", "seterase", "kfbadflag", "cullkfs")
ID_LIMIT = 1 << 31
MAX_CULL_LIST = 4096
NOTHING, DEFERRED, DONE = 0, 1, 2       # ORBFE_MAP_BAD_*
KEPT, CULLED, DEFERRED_CULL = 0, 1, 2   # ORBFE_MAP_CULL_*


def _bits(depths):
    """float32 values as their bit patterns: -0 and NaN compare as what they are."""
    return [int(x) for x in np.asarray(depths, np.float32).view(np.uint32)]


class Refused(Exception):
    """What the library answers with ORBFE_ERR_ARG; nothing has changed."""


class Capacity(Exception):
    """ORBFE_ERR_CAPACITY; nothing has changed."""


class Model(K.Model):
    """covis_cases.Model plus, per keyframe: octave, right, depth (one per slot), th_depth; per
    point: obs as {keyframe: idx or None}, nobs, found, visible, first."""

    def apply(self, op):
        k = op[0]
        if k == "points":
            super().apply(op)
            for n in op[1]:
                mp = self.mps[n]
                mp.obs, mp.nobs, mp.found, mp.visible, mp.first = {}, 0, 1, 1, 0   # MapPoint.cc:37-38
        elif k == "kf":
            super().apply(op)
            kf = self.kfs[op[1]]
            n = len(kf.mps)
            kf.octave, kf.right, kf.depth, kf.th_depth = [0] * n, [False] * n, [-1.0] * n, 0.0
            kf.not_erase, kf.to_erase = False, False                       # KeyFrame.cc:42
        elif k == "obs":
            for p, f in op[1]:
                self.add_observation(p, f, None)
        elif k == "unobs":
            for p, f in op[1]:
                self.erase_plain(p, f)
        else:
            super().apply(op)

    def _by(self, kf, idx, mutant, which):
        right = idx is not None and self.kfs[kf].right[idx]                # :346, :360
        if mutant == which:
            right = False
        return 2 if right else 1

    # ---- MapPoint.cc:339-350
    def add_observation(self, p, kf, idx, mutant=None, st=None):
        mp = self.mps[p]
        if idx is not None and not 0 <= idx < len(self.kfs[kf].mps):
            raise Refused("idx")
        if kf in mp.obs:                                                   # :342
            _bump(st, "add_present")
            if mutant == "add_overwrites":
                mp.obs[kf] = idx
            return
        mp.obs[kf] = idx                                                   # :344
        by = self._by(kf, idx, mutant, "right_ignored")
        _bump(st, "add_right" if by == 2 else "add_left_only")
        mp.nobs += by                                                      # :346-349

    def erase_plain(self, p, kf):
        """The library's batched erase: the set and nObs, no `nObs <= 2` rule."""
        mp = self.mps[p]
        if kf in mp.obs:
            mp.nobs -= self._by(kf, mp.obs[kf], None, "-")
            del mp.obs[kf]

    # ---- MapPoint.cc:352-378
    def erase_observation(self, p, kf, mutant=None, st=None):
        mp = self.mps[p]
        if kf not in mp.obs:                                               # :357
            _bump(st, "erase_absent")
            return False
        by = self._by(kf, mp.obs[kf], mutant, "erase_right_ignored")       # :359-363
        _bump(st, "erase_right" if by == 2 else "erase_left_only")
        left = mp.nobs - by
        bad = left < 2 if mutant == "bad_lt2" else left <= 2               # :371
        if mutant == "erase_never_bad":
            bad = False
        if bad and any(i is None for f, i in mp.obs.items() if f != kf):
            raise Refused("an index is unknown")
        mp.nobs = left
        del mp.obs[kf]                                                     # :365
        if bad:
            _bump(st, "erase_to_bad")
            self.set_bad_flag(p, mutant, st)                               # :377
        else:
            _bump(st, "erase_stays")
        return bad

    # ---- MapPoint.cc:392-409
    def set_bad_flag(self, p, mutant=None, st=None):
        mp = self.mps[p]
        if any(i is None for i in mp.obs.values()):
            raise Refused("an index is unknown")
        mp.bad = True                                                      # :398
        obs = dict(mp.obs)                                                 # :399
        if mutant != "badflag_keeps_obs":
            mp.obs = {}                                                    # :400
        if mutant == "badflag_resets_nobs":
            mp.nobs = 0
        _bump(st, "badflag_empty" if not obs else "badflag_observed")
        for kf, idx in obs.items():                                        # :402
            held = self.kfs[kf].mps[idx]
            _bump(st, "match_is_point" if held == p else "match_null" if held is None else "match_other")
            if mutant == "match_checked" and held != p:
                continue
            self.kfs[kf].mps[idx] = None                                   # :405, EraseMapPointMatch(idx)

    def found_ratio(self, p, mutant=None):
        mp = self.mps[p]
        if mutant == "ratio_double":
            with np.errstate(divide="ignore", invalid="ignore"):
                return np.float64(mp.found) / np.float64(mp.visible)
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.float32(mp.found) / np.float32(mp.visible)           # static_cast<float>(mnFound)/mnVisible

    # ---- LocalMapping.cc:170-205
    def cull_points(self, lst, cur, mono, mutant=None, st=None):
        if not 0 <= cur < ID_LIMIT:
            raise Refused("current id")
        for p in lst:
            if not self.mps[p].bad and not 0 <= self.mps[p].first < ID_LIMIT:
                raise Refused("first id")
        th = 2 if mono or mutant == "th_obs_2" else 3                      # :176-181
        if mutant == "dup_independent":
            frozen = {p: self.mps[p].bad for p in lst}
        kept, culled = [], []
        # a refusal comes before anything changes: SetBadFlag runs after the loop, and a point
        # it will run on counts as bad from its position on
        for p in lst:                                                      # :183
            mp = self.mps[p]
            is_bad = mp.bad or p in culled
            if mutant == "dup_independent":
                is_bad = frozen[p]
            diff = int(cur) - int(mp.first)
            ratio = self.found_ratio(p, mutant)
            low = ratio <= 0.25 if mutant == "ratio_le" else ratio < np.float32(0.25)
            few = mp.nobs < th if mutant == "nobs_lt" else mp.nobs <= th
            young = diff > 2 if mutant == "diff_gt" else diff >= 2
            if is_bad:                                                     # :186
                _bump(st, "cull_was_bad" if mp.bad else "cull_repeated")
                if mutant == "bad_listed_kept":
                    kept.append(p)
            elif low:                                                      # :190
                _bump(st, "cull_ratio" if np.isfinite(ratio) else "cull_ratio_neg_inf")
                culled.append(p)
            elif mutant == "branch_order" and diff >= 3:
                _bump(st, "cull_old")
            elif young and few:                                            # :195
                _bump(st, "cull_few_obs")
                culled.append(p)
            elif diff >= 3 and mutant != "old_kept":                       # :200
                _bump(st, "cull_old")
            else:
                _bump(st, "cull_kept_nan" if np.isnan(ratio) else "cull_kept_inf" if np.isinf(ratio)
                      else "cull_kept")
                kept.append(p)
        for p in dict.fromkeys(culled):
            if any(i is None for i in self.mps[p].obs.values()):
                raise Refused("an index is unknown")
        for p in culled:
            self.set_bad_flag(p, mutant, st)                               # :192, :197
        return kept, culled

    # ---- KeyFrame.cc:971-996
    def tracked(self, kf, min_obs, mutant=None, st=None):
        n = 0
        check = min_obs > 0                                                # :976
        for p in self.kfs[kf].mps:                                         # :977
            if p is None:                                                  # :980
                _bump(st, "tracked_null")
                continue
            mp = self.mps[p]
            if mp.bad and mutant != "tracked_counts_bad":                  # :982
                _bump(st, "tracked_bad")
                continue
            if check and mutant != "tracked_ignores_obs":                  # :984
                ok = mp.nobs > min_obs if mutant == "tracked_gt" else mp.nobs >= min_obs   # :986
                _bump(st, "tracked_enough" if ok else "tracked_too_few")
                n += ok
            else:
                _bump(st, "tracked_unchecked")
                n += 1
        return n

    # ---- KeyFrame.cc:1174-1287
    def _kf_refusal(self, name, mutant=None):
        """A point that the erase would set bad while another observer of it has no index."""
        kf = self.kfs[name]
        for p in dict.fromkeys(q for q in kf.mps if q is not None):
            mp = self.mps[p]
            if name not in mp.obs:
                continue
            by = self._by(name, mp.obs[name], None, "-")
            if mp.nobs - by <= 2 and any(i is None for f, i in mp.obs.items() if f != name):
                raise Refused("an index is unknown")

    def kf_set_bad_flag(self, name, is_first, mutant=None, st=None, bad=None, pairs=None):
        kf = self.kfs[name]
        bad = [] if bad is None else bad
        pairs = [] if pairs is None else pairs
        if is_first:                                                       # :1179
            _bump(st, "kfbad_first")
            return NOTHING
        if kf.not_erase and mutant != "noterase_ignored":                  # :1181
            _bump(st, "kfbad_deferred")
            kf.to_erase = True
            return DEFERRED
        self._kf_refusal(name, mutant)
        if mutant != "conn_after_tree":
            self.erase_keyframe(name, mutant, st)                          # :1188-1189 (:1198-1199 early: nothing reads them between)
        for i, p in enumerate(kf.mps):                                     # :1191
            if p is None:
                continue
            mp = self.mps[p]
            if name not in mp.obs:                                         # MapPoint.cc:357
                _bump(st, "kfbad_second_index" if p in kf.mps[:i] else "kfbad_not_listed")
                continue
            idx = mp.obs[name]
            right = idx is not None and kf.right[i if mutant == "right_at_i" else idx]   # MapPoint.cc:360
            _bump(st, "kfbad_right" if right else "kfbad_left_only")
            mp.nobs -= 2 if right else 1
            del mp.obs[name]
            if mp.nobs < 2 if mutant == "kf_bad_lt2" else mp.nobs <= 2:    # MapPoint.cc:371
                _bump(st, "kfbad_point_bad")
                self.set_bad_flag(p, mutant, st)
                bad.append(p)
            else:
                _bump(st, "kfbad_point_stays")
        cands = set()                                                      # :1202
        if kf.parent is not None:
            cands.add(kf.parent)
        else:
            _bump(st, "kfbad_no_parent")
        while kf.children:                                                 # :1208
            mx, pc, pp = -1, None, None
            for c in sorted(kf.children, key=self.key):                    # :1216, pointer order
                ck = self.kfs[c]
                if ck.bad and mutant != "bad_child_reassigned":            # :1222
                    _bump(st, "tree_bad_child")
                    continue
                for pos, o in enumerate(ck.ordered):                       # :1230
                    if o not in cands:                                     # :1238
                        continue
                    if o not in ck.weights:
                        _bump(st, "tree_listed_without_weight")
                    w = ck.weights.get(o, 0)                               # GetWeight: the weight map
                    if mutant == "tournament_ordered_weights":
                        w = ck.oweights[pos]
                    if w == mx:
                        _bump(st, "tree_tie")
                    if w > mx or (mutant == "tournament_ge" and w >= mx):  # :1243
                        mx, pc, pp = w, c, o
            if pc is None:                                                 # :1263
                _bump(st, "tree_no_candidate")
                break
            _bump(st, "tree_reassigned")
            self.kfs[pc].parent = pp                                       # :1259, ChangeParent
            self.kfs[pp].children.add(pc)
            pairs.append((pc, pp))
            cands.add(pc)                                                  # :1260
            kf.children.discard(pc)                                        # :1261
        if kf.children:                                                    # :1268
            for c in sorted(kf.children, key=self.key):
                if kf.parent is not None:                                  # :1272
                    _bump(st, "tree_leftover_bad" if self.kfs[c].bad else "tree_leftover")
                    self.kfs[c].parent = kf.parent
                    self.kfs[kf.parent].children.add(c)
                    pairs.append((c, kf.parent))
                else:
                    _bump(st, "tree_orphan")
            if mutant == "children_cleared":
                kf.children = set()
        if kf.parent is not None:
            self.kfs[kf.parent].children.discard(name)                     # :1277
        kf.bad = True                                                      # :1281
        if mutant == "conn_after_tree":
            self.erase_keyframe(name, mutant, st)
        return DONE

    # ---- KeyFrame.cc:1158-1172
    def set_erase(self, name, has_loop_edges, is_first, mutant=None, st=None, bad=None, pairs=None):
        kf = self.kfs[name]
        if kf.to_erase and not (kf.not_erase and has_loop_edges) and not is_first:
            self._kf_refusal(name, mutant)
        if not has_loop_edges and mutant != "seterase_keeps_flag":         # :1162
            kf.not_erase = False
        if kf.to_erase:                                                    # :1168
            _bump(st, "seterase_runs")
            return self.kf_set_bad_flag(name, is_first, mutant, st, bad, pairs)
        _bump(st, "seterase_plain")
        return NOTHING

    # ---- LocalMapping.cc:643-695
    def cull_decision(self, name, mono, mutant=None, st=None):
        kf = self.kfs[name]
        th_obs = 2 if mutant == "kf_th_obs_2" else 3                       # :649
        n_mps = n_red = 0
        seen = set()
        for i, p in enumerate(kf.mps):                                     # :653
            if p is None:                                                  # :656
                continue
            mp = self.mps[p]
            if mp.bad and mutant != "bad_point_in_nmps":                   # :658
                _bump(st, "dec_bad_point")
                continue
            if p in seen:
                _bump(st, "dec_held_twice")
                if mutant == "held_twice_counts_once":
                    continue
            seen.add(p)
            if not mono or mutant == "depth_in_mono":                      # :660
                z, th = np.float32(kf.depth[i]), np.float32(kf.th_depth)
                far = z >= th if mutant == "depth_ge" else z > th
                if far or z < 0:                                           # :662
                    _bump(st, "dec_far" if far else "dec_negative")
                    continue
                if np.isnan(z) or (z == 0 and np.signbit(z)):
                    _bump(st, "dec_nan_or_minus_zero")
            n_mps += 1                                                     # :666
            if mp.nobs > th_obs:                                           # :667
                level = kf.octave[i]
                n = 0
                for o, idx in mp.obs.items():                              # :672
                    if o == name and mutant != "self_counted":             # :675
                        continue
                    lj = self.kfs[o].octave[idx]
                    if lj == level + 1:
                        _bump(st, "dec_octave_edge")
                    if lj <= level + (0 if mutant == "octave_plus_0" else 1):   # :679
                        n += 1
                        if n >= th_obs:
                            break
                if n >= th_obs:                                            # :686
                    n_red += 1
                else:
                    _bump(st, "dec_not_redundant")
            else:
                _bump(st, "dec_few_obs")
        if n_mps == 0:
            _bump(st, "dec_no_points")
        out = n_red >= 0.9 * n_mps if mutant == "cull_ge" else n_red > 0.9 * n_mps   # :695
        _bump(st, "dec_cull" if out else "dec_keep")
        return out

    def _cull_list(self, cur, lst):
        lst = list(self.kfs[cur].ordered) if lst is None else list(lst)    # :638, a copy
        if len(lst) > MAX_CULL_LIST:
            raise Capacity()
        if any(i is None for mp in self.mps.values() for i in mp.obs.values()):
            raise Refused("an index is unknown")
        return lst

    def cull_keyframes(self, cur, lst, first, mono, mutant=None, st=None):
        """The reference's sequential loop -> (list, results, bad points, pairs)."""
        lst = self._cull_list(cur, lst)
        res, bad, pairs = [], [], []
        if mutant == "one_shot":
            frozen = [n != first and self.cull_decision(n, mono, mutant) for n in lst]
        for j, n in enumerate(lst):                                        # :640
            if n == first and mutant != "first_culled":                    # :643
                _bump(st, "cull_first_skipped")
                res.append(KEPT)
                continue
            if frozen[j] if mutant == "one_shot" else self.cull_decision(n, mono, mutant, st):
                if any(r == CULLED for r in res):
                    _bump(st, "cull_after_a_cull")
                what = self.kf_set_bad_flag(n, False, mutant, st, bad, pairs)   # :696
                res.append(CULLED if what == DONE else DEFERRED_CULL)
            else:
                res.append(KEPT)
        return lst, res, bad, pairs

    def cull_keyframes_rounds(self, cur, lst, first, mono):
        """The scheme the library runs: every keyframe not yet passed decides on the map as it
        stands; the first that culls is applied; the ones after it decide again."""
        lst = self._cull_list(cur, lst)
        res, bad, pairs = [KEPT] * len(lst), [], []
        start, rounds = 0, 0
        while start < len(lst):
            rounds += 1
            dec = [n != first and self.cull_decision(n, mono) for n in lst[start:]]
            j = start
            while j < len(lst):
                if dec[j - start]:
                    what = self.kf_set_bad_flag(lst[j], False, None, None, bad, pairs)
                    res[j] = CULLED if what == DONE else DEFERRED_CULL
                    if what == DONE:
                        break
                j += 1
            start = j + 1
        return (lst, res, bad, pairs), rounds

    def state(self):
        """(keyframes: name -> (mvpMapPoints, bad, not-erase, to-be-erased); points: name -> (bad,
        [(kf, idx)] by keyframe slot, nObs, found, visible, first); the graph and the spanning
        tree as covis_cases has them)."""
        kfs = {n: (list(kf.mps), bool(kf.bad), bool(kf.not_erase), bool(kf.to_erase))
               for n, kf in self.kfs.items()}
        mps = {n: (bool(mp.bad), sorted(mp.obs.items(), key=lambda e: self.kfs[e[0]].slot), mp.nobs,
                   mp.found, mp.visible, mp.first) for n, mp in self.mps.items()}
        return kfs, mps, self.graph()

    def run(self, op, mutant=None, st=None):
        k = op[0]
        out = None
        try:
            if k == "features":
                kf = self.kfs[op[1]]
                n = len(kf.mps)
                if op[2] is not None and not all(0 <= o < 128 for o in op[2]):
                    raise Refused("octave")
                if any(a is not None and len(a) != n for a in op[2:5]):
                    raise Refused("one entry per slot")
                kf.octave = list(op[2]) if op[2] is not None else [0] * n
                kf.right = [bool(u >= 0) for u in op[3]] if op[3] is not None else [False] * n
                kf.depth = [float(np.float32(d)) for d in op[4]] if op[4] is not None else [-1.0] * n
                kf.th_depth = float(np.float32(op[5]))
                return (list(kf.octave), list(kf.right), _bits(kf.depth), kf.th_depth), None
            elif k == "obsidx":
                for p, f, i in op[1]:
                    if not 0 <= i < len(self.kfs[f].mps):
                        raise Refused("idx")
                for p, f, i in op[1]:
                    self.add_observation(p, f, i, mutant, st)
            elif k == "eraseobs":
                out = self.erase_observation(op[1], op[2], mutant, st)
            elif k == "counters":
                for j, p in enumerate(op[1]):
                    mp = self.mps[p]
                    for attr, vals in zip(("nobs", "found", "visible", "first"), op[2:6]):
                        if vals is not None:
                            setattr(mp, attr, vals[j])
            elif k == "inc":
                for j, p in enumerate(op[2]):
                    a = 1 if op[3] is None else op[3][j]
                    mp = self.mps[p]
                    if op[1] == "found":
                        mp.found += a
                    else:
                        mp.visible += a
            elif k == "mpbadflag":
                for p in op[1]:
                    if any(i is None for i in self.mps[p].obs.values()):
                        raise Refused("an index is unknown")
                for p in dict.fromkeys(op[1]):
                    self.set_bad_flag(p, mutant, st)
            elif k == "cullpoints":
                out = self.cull_points(list(op[1]), op[2], op[3], mutant, st)
            elif k == "tracked":
                out = self.tracked(op[1], op[2], mutant, st)
            elif k == "noterase":
                self.kfs[op[1]].not_erase = bool(op[2])
            elif k == "kfbadflag":
                bad, pairs = [], []
                what = self.kf_set_bad_flag(op[1], bool(op[2]) if len(op) > 2 else False, mutant, st, bad, pairs)
                out = (what, bad, pairs)
            elif k == "seterase":
                bad, pairs = [], []
                what = self.set_erase(op[1], bool(op[2]), bool(op[3]) if len(op) > 3 else False, mutant, st,
                                      bad, pairs)
                out = (what, bad, pairs)
            elif k == "cullkfs":        # ("cullkfs", current, list|None, first|None, monocular)
                out = self.cull_keyframes(op[1], op[2], op[3], op[4], mutant, st)
            elif k in K.OPS or k == "localmap":
                return super().run(op, mutant, st)
            else:
                self.apply(op)
                return None
        except Refused:
            return "error", self.state()
        except Capacity:
            return "capacity", self.state()
        return out, self.state()


def run_script(script, mutant=None, stats=None):
    m, out = Model(), []
    for op in script:
        a = m.run(op, mutant, stats)
        if a is not None:
            out.append(a)
    return out


# ---- the driver over native.LocalMap -----------------------------------------------------------
class LibraryRunner(K.LibraryRunner):
    """Replays a script on a ``native.LocalMap``; after every culling operation the whole state is
    read back through the getters.  `batch`: "batch" (one call per operation) or "single" (one
    call per element where the operation is a batch)."""

    def state(self):
        lm, kn, pn = self.lm, self.kf_names, self.mp_names
        kbad = lm.get_bad_flags(0, list(range(len(kn))))
        kfs = {n: ([None if s < 0 else pn[s] for s in lm.get_keyframe_points(i)], bool(kbad[i]),
                   *lm.get_erase_flags(i)) for i, n in enumerate(kn)}
        pbad = lm.get_bad_flags(1, list(range(len(pn))))
        o, f, v, first = lm.get_point_counters(list(range(len(pn))))
        mps = {}
        for i, n in enumerate(pn):
            ks, xs = lm.GetObservations(i)
            mps[n] = (bool(pbad[i]), [(kn[a], None if b < 0 else int(b)) for a, b in zip(ks, xs)],
                      int(o[i]), int(f[i]), int(v[i]), int(first[i]))
        return kfs, mps, self.graph()

    def _report(self, what, bad, pairs):
        return (int(what), [self.mp_names[p] for p in bad],
                [(self.kf_names[a], self.kf_names[b]) for a, b in pairs])

    def _chunks(self, items):
        return [items] if self.batch == "batch" else [[x] for x in items]

    def apply(self, op):
        from orbslam_mapsave_amd import abi
        k, lm = op[0], self.lm
        out = None
        try:
            if k == "features":
                lm.set_keyframe_features(self.kf[op[1]], op[2], op[3], op[4], op[5])
                o, r, d, th = lm.get_keyframe_features(self.kf[op[1]])
                return ([int(x) for x in o], [bool(x) for x in r], _bits(d), float(th)), None
            elif k == "obsidx":
                if self.batch != "batch":   # all or nothing, as the batch is
                    for p, f, i in op[1]:
                        if not 0 <= i < len(lm.get_keyframe_points(self.kf[f])):
                            raise abi.OrbfeError("idx", abi.ORBFE_ERR_ARG)
                for c in self._chunks(op[1]):
                    lm.AddObservation([self.mp[p] for p, _, _ in c], [self.kf[f] for _, f, _ in c],
                                      [i for _, _, i in c])
            elif k == "eraseobs":
                out = lm.EraseObservation(self.mp[op[1]], self.kf[op[2]])
            elif k == "counters":
                lm.set_point_counters([self.mp[p] for p in op[1]], *op[2:6])
            elif k == "inc":
                fn = lm.IncreaseFound if op[1] == "found" else lm.IncreaseVisible
                if self.batch == "batch":
                    fn([self.mp[p] for p in op[2]], op[3])
                else:
                    for j, p in enumerate(op[2]):
                        fn(self.mp[p], None if op[3] is None else op[3][j])
            elif k == "mpbadflag":
                if self.batch != "batch":
                    for p in op[1]:
                        if (lm.GetObservations(self.mp[p])[1] < 0).any():
                            raise abi.OrbfeError("idx", abi.ORBFE_ERR_ARG)
                for c in self._chunks(op[1]):
                    lm.SetMapPointBadFlag([self.mp[p] for p in c])
            elif k == "cullpoints":
                kept, gone = lm.MapPointCulling([self.mp[p] for p in op[1]], op[2], op[3])
                out = ([self.mp_names[s] for s in kept], [self.mp_names[s] for s in gone])
            elif k == "tracked":
                out = lm.TrackedMapPoints(self.kf[op[1]], op[2])
            elif k == "noterase":
                lm.SetNotErase(self.kf[op[1]], op[2])
            elif k == "kfbadflag":
                out = self._report(*lm.SetKeyFrameBadFlag(self.kf[op[1]], bool(op[2]) if len(op) > 2 else False))
            elif k == "seterase":
                out = self._report(*lm.SetErase(self.kf[op[1]], bool(op[2]), bool(op[3]) if len(op) > 3 else False))
            elif k == "cullkfs":
                lst, res, bad, pairs = lm.KeyFrameCulling(
                    self.kf[op[1]], op[4], None if op[2] is None else [self.kf[n] for n in op[2]],
                    -1 if op[3] is None else self.kf[op[3]])
                out = ([self.kf_names[x] for x in lst], [int(x) for x in res]) + self._report(0, bad, pairs)[1:]
            else:
                return super().apply(op)
        except abi.OrbfeError as e:
            if e.status == abi.ORBFE_ERR_CAPACITY:
                return "capacity", self.state()
            assert e.status == abi.ORBFE_ERR_ARG, e
            return "error", self.state()
        return out, self.state()


# ---- built cases -------------------------------------------------------------------------------
def _map(v, nkf, slots, right_every=3):
    """nkf keyframes of `slots` slots and one point per (keyframe, slot) diagonal: point p_j is held
    at slot j of every keyframe; keyframe i has a right coordinate at every slot j with
    (i + j) % right_every == 0."""
    s = []
    pts = [f"p{j}" for j in range(slots)]
    s.append(("points", pts))
    names = [f"K{i}" for i in range(nkf)]
    for n, key in zip(names, keys_for(nkf, v)):
        s.append(("kf", n, key, list(pts)))
    for i, n in enumerate(names):
        s.append(("features", n, [(i + j) % 8 for j in range(slots)],
                  [float(j) if (i + j) % right_every == 0 else -1.0 for j in range(slots)],
                  [0.5 * j for j in range(slots)], 35.0 + v))
    return s, names, pts


def case_observations(v):
    """AddObservation with and without a right coordinate, a pair added twice (the index stays),
    the index-less call, the batched erase, EraseObservation landing on nObs 3, 2 and 1, on an
    absent pair, with a right coordinate at the observation's index."""
    s, names, pts = _map(v, 5, 8)
    s.append(("obsidx", [(p, n, j) for j, p in enumerate(pts) for n in names[:4]]))
    s.append(("obsidx", [(pts[0], names[0], 5), (pts[1], names[4], 1)]))      # present: no-op; new
    s.append(("obs", [(pts[2], names[4]), (pts[2], names[0])]))                # index unknown / present
    s.append(("unobs", [(pts[2], names[4]), (pts[3], names[4]), (pts[3], names[1])]))
    s.append(("obsidx", [(pts[0], names[1], 99)]))                             # refused
    s.append(("obsidx", [(pts[4], names[4], 4), (pts[5], names[0], -1)]))      # all or nothing
    for p in pts[:4]:
        for n in names[:4]:
            s.append(("eraseobs", p, n))
    s.append(("eraseobs", pts[0], names[0]))                                   # already bad, absent
    s.append(("kfpoints", names[3], 6, [pts[7]]))                              # slot 6 holds p7 now
    s.append(("eraseobs", pts[6], names[v % 3]))
    s.append(("eraseobs", pts[6], names[(v + 1) % 3]))                         # p6 goes bad: K3[6] erased whatever it holds
    return s


def case_badflag(v):
    """SetBadFlag: the entry erased whatever it holds (this point, another, NULL), nObs kept, a
    point with no observers, a point listed twice, an unknown index refused before anything."""
    s, names, pts = _map(v, 4, 6)
    s.append(("obsidx", [(p, n, j) for j, p in enumerate(pts) for n in names]))
    s.append(("kfpoints", names[0], 1, [pts[2]]))          # K0[1] holds p2, p1 still observes K0 at 1
    s.append(("kfpoints", names[1], 1, [None]))
    s.append(("mpbadflag", [pts[1]]))
    s.append(("points", ["lonely"]))
    s.append(("mpbadflag", ["lonely", pts[3], pts[3]]))
    s.append(("unobs", [(pts[4], names[2])]))
    s.append(("obs", [(pts[4], names[2])]))                # back, index unknown
    s.append(("mpbadflag", [pts[5], pts[4]]))              # refused: p5 stays too
    s.append(("mpbadflag", [pts[5]]))
    s.append(("eraseobs", pts[4], names[3]))               # nObs high enough: stays
    s.append(("counters", [pts[4]], [3], None, None, None))
    s.append(("eraseobs", pts[4], names[0]))               # would go bad with an unknown index: refused
    s.append(("tracked", names[0], 0))
    return s


def case_cullpoints(v):
    """Every branch of MapPointCulling at its edge: ratio 0.25 and its neighbours, visible 0 with
    found 0 / 1 / negative, the id difference at 1, 2, 3, nObs at the threshold and beside it in
    mono and stereo, bad points, a point listed twice in every branch, float rounding of the ratio."""
    s, names, pts = _map(v, 4, 40)
    s.append(("obsidx", [(p, n, j) for j, p in enumerate(pts) for n in names]))
    cur = 10 + v
    mono = bool(v % 2)
    th = 2 if mono else 3
    rows = [  # (found, visible, first, nobs)
        (1, 4, cur, 9), (1, 5, cur, 9), (249999, 1000000, cur, 9), (250001, 1000000, cur, 9),
        (0, 0, cur, 9), (1, 0, cur, 9), (-1, 0, cur, 9), (0, 7, cur, 9),
        (1 << 24, (1 << 26) + 1, cur, 9), (1 << 24, (1 << 26) + 8, cur, 9),
        (5, 5, cur - 1, th), (5, 5, cur - 2, th), (5, 5, cur - 2, th + 1), (5, 5, cur - 2, th - 1),
        (5, 5, cur - 3, th + 1), (5, 5, cur - 3, th), (5, 5, cur - 2, 2), (5, 5, cur - 2, 3),
        (5, 5, cur + 4, 0), (5, 5, 0, 50), (1, 5, cur - 3, 0), (5, 5, cur - 1, 0),
    ]
    use = pts[:len(rows)]
    s.append(("counters", use, [r[3] for r in rows], [r[0] for r in rows], [r[1] for r in rows],
              [r[2] for r in rows]))
    s.append(("mpbad", [pts[30]], True))
    lst = use + [pts[30]] + use[::3] + [pts[31]]
    if v % 3 == 1:
        lst = lst[::-1]
    s.append(("cullpoints", lst, cur, mono))
    s.append(("cullpoints", lst, cur, mono))               # what is left, again
    s.append(("cullpoints", [], cur, mono))
    s.append(("cullpoints", [pts[32]], cur + 3, not mono))
    s.append(("counters", [pts[33]], None, None, None, [ID_LIMIT]))
    s.append(("cullpoints", [pts[34], pts[33]], cur, mono))   # refused
    s.append(("cullpoints", [pts[34]], ID_LIMIT, mono))       # refused
    s.append(("counters", [pts[33]], None, None, None, [ID_LIMIT - 1]))
    s.append(("cullpoints", [pts[34], pts[33]], ID_LIMIT - 1, mono))
    s.append(("unobs", [(pts[35], names[0])]))
    s.append(("obs", [(pts[35], names[0])]))
    s.append(("counters", [pts[35], pts[36]], None, [0, 0], [9, 9], None))
    s.append(("cullpoints", [pts[36], pts[35]], cur, mono))   # a culled point with an unknown index: refused
    s.append(("cullpoints", [pts[36]], cur, mono))
    return s


def case_counters(v):
    """IncreaseFound / IncreaseVisible with and without amounts, a repeated point, the ratio they
    lead to; TrackedMapPoints at min_obs 0 .. 4 over NULL, bad and thinly observed points."""
    s, names, pts = _map(v, 3, 12, right_every=2)
    s.append(("obsidx", [(p, n, j) for j, p in enumerate(pts[:10]) for n in names[:1 + j % 3]]))
    s.append(("inc", "found", pts[:4] + pts[:2], None))
    s.append(("inc", "visible", pts[:6], [3, 0, 7 + v, 1, -1, 2]))
    s.append(("inc", "visible", [pts[0], pts[0], pts[0]], [1, 2, 3]))
    s.append(("kfpoints", names[0], 10, [None]))
    s.append(("mpbad", [pts[1]], True))
    for mo in (-1, 0, 1, 2, 3, 4, 5):
        s.append(("tracked", names[0], mo))
    s.append(("tracked", names[2], 1))
    s.append(("cullpoints", pts, 1, False))
    s.append(("clear",))
    t, names, pts = _map(v + 1, 2, 3)
    s.extend(t)
    s.append(("obsidx", [(pts[0], names[0], 0)]))
    s.append(("cullpoints", pts, 2, True))
    return s


def case_kfbadflag(v):
    """KeyFrame::SetBadFlag: mnId == 0, not-erase and SetErase with and without loop edges, a point
    held at two indices, held without being listed, the right flag at the observation's index,
    points landing on nObs 3 / 2, the tournament with a tie between children and within a list, a
    candidate listed without a weight, a bad child, a child that finds a candidate only through the
    erase's re-sort, no parent, leftover children with and without a parent."""
    s, names, pts = _map(v, 9, 30)
    K0, K1, K2, K3, K4, K5, K6, K7, K8 = names
    s.append(("obsidx", [(p, n, (j + 1) % 30 if (i, j) == (1, 7) else j) for j, p in enumerate(pts)
                         for i, n in enumerate(names) if (i + j) % 5 != 4 and (i < 4 or j % 3 == v % 3)]))
    s.append(("update_batch", names))
    tree = {K0: None, K1: K0, K2: K1, K3: K1, K4: K1, K5: K2, K6: None, K7: K6, K8: K1}
    for n, par in tree.items():
        s.append(("parent", n, par))
        s.append(("children", n, [c for c, q in tree.items() if q == n]))
    s.append(("kfpoints", K1, 0, [pts[5]]))                  # p5 at 0 and 5
    s.append(("kfbad", K3, True))
    # K4 lists no candidate until K1 leaves its weight map; K2 and K3 tie towards K0
    s.append(("setconn", K4, [(K1, 20), (K2, 5), (K6, 30)]))
    s.append(("setordered", K4, [(K6, 30), (K1, 20)]))
    # K2 is not in K1's way (no re-sort): its list's weights are not the map's; K8 competes with it
    s.append(("setconn", K2, [(K0, 9 + v % 2), (K5, 9)]))
    s.append(("setordered", K2, [(K5, 2), (K0, 1)]))
    s.append(("setconn", K8, [(K0, 5)]))
    s.append(("setordered", K8, [(K0, 5)]))
    s.append(("kfbadflag", K0, True))
    s.append(("noterase", K1, True))
    s.append(("kfbadflag", K1))
    s.append(("seterase", K1, True))
    s.append(("seterase", K7, False))                        # nothing pending
    s.append(("seterase", K1, False))
    s.append(("kfbadflag", K6))                              # no parent: K7 keeps it
    s.append(("setordered", K5, [(K7, 4), (K0, 0)]))         # K0 listed, not in the weight map
    s.append(("setconn", K5, [(K7, 4)]))
    s.append(("kfbadflag", K2))
    s.append(("kfbadflag", K2))                              # again, on a bad keyframe
    s.append(("kfbadflag", K0))                              # every child left over, no parent
    s.append(("tracked", K4, 1))
    return s


class _World:
    """Keyframes built for KeyFrameCulling: helpers H0..H3 whose slots are handed out one by one."""

    def __init__(self, v, helpers=4, helper_slots=400):
        self.s, self.v = [], v
        self.helpers = [f"H{i}" for i in range(helpers)]
        self.used = {h: 0 for h in self.helpers}
        self.hs = helper_slots
        self.pts, self.kfs, self.obs = [], [], []
        self.feat = {h: ([0] * helper_slots, [-1.0] * helper_slots, [1.0] * helper_slots, 40.0)
                     for h in self.helpers}
        self.held = {h: [None] * helper_slots for h in self.helpers}

    def point(self, name, holders):
        """holders: [(kf, slot, octave)]; helper slots are given as None."""
        self.pts.append(name)
        for kf, slot, octave in holders:
            if slot is None:
                slot = self.used[kf]
                self.used[kf] += 1
            self.held[kf][slot] = name
            self.feat[kf][0][slot] = octave
            self.obs.append((name, kf, slot))

    def keyframe(self, name, slots, depth=None, th=40.0, right=None):
        self.kfs.append(name)
        self.held[name] = [None] * slots
        self.feat[name] = ([0] * slots, right or [-1.0] * slots, depth or [1.0] * slots, th)

    def script(self):
        s = [("points", self.pts)]
        names = self.helpers + self.kfs
        for n, key in zip(names, keys_for(len(names), self.v)):
            s.append(("kf", n, key, self.held[n]))
            s.append(("features", n, *self.feat[n]))
        s.append(("obsidx", self.obs))
        return s

    def redundant_points(self, kf, tag, n, n_red, octave=1, first=0, via=None):
        """n points held by kf at slots first..: n_red of them seen by three more keyframes at an
        octave <= octave + 1 (one exactly there), the rest by three of which one is at octave + 2."""
        via = via or self.helpers[:3]
        for i in range(n):
            levels = (octave, octave + 1, octave + 1) if i < n_red else (octave, octave + 1, octave + 2)
            self.point(f"{tag}{i}", [(kf, first + i, octave)] + [(h, None, l) for h, l in zip(via, levels)])


def case_cullkfs(v):
    """KeyFrameCulling at its edges: nMPs 10 with 9 and 10 redundant, 20 with 18 and 19, nMPs 0; a
    first cull that flips a later keyframe from culled to kept, and one from kept to culled through
    a point going bad; observers' octaves at +1 and +2; a point held twice; the mnId == 0 keyframe
    listed; a not-erase keyframe deferred and culled later by SetErase; stereo depth on mThDepth,
    its neighbours, -0, a negative, NaN, +inf."""
    w = _World(v)
    for name, n, r in (("A", 10, 10), ("B9", 10, 9), ("C", 20, 19), ("D18", 20, 18), ("E0", 5, 0),
                       ("D2", 20, 18)):
        w.keyframe(name, n + 3)
        w.redundant_points(name, name.lower() + "_", n, r)
    w.held["D2"][20] = "d2_0"                                 # held twice: counted twice, 19 of 21
    w.feat["D2"][0][20] = 1
    w.held["E0"] = [None] * 8                                 # nMPs 0
    w.obs = [o for o in w.obs if o[1] != "E0"]
    # F: redundant only while A observes its points (A, H0, H1 + F: nObs 4 -> 3 once A is gone)
    w.keyframe("F", 10)
    for i in range(10):
        w.point(f"f_{i}", [("F", i, 1), ("A", 10 if i == 0 else 11, 1), ("H0", None, 1), ("H1", None, 2)][:4]
                if i < 2 else [("F", i, 1), ("H0", None, 1), ("H1", None, 2), ("H2", None, 1)])
    # G: 9 of 10 redundant; g_q is seen by A, G and H0 only: A's erase leaves nObs 2, it goes bad
    w.keyframe("G", 12)
    w.redundant_points("G", "g_", 9, 9)
    w.keyframe("A2", 3)
    w.point("g_q", [("G", 9, 1), ("A", 12, 1), ("H0", None, 1)])
    # depth: stereo only
    th = np.float32(2.5)
    z = [th, np.nextafter(th, np.float32(9)), np.nextafter(th, np.float32(0)), np.float32(-0.0),
         np.float32(-1e-3), np.float32(np.nan), np.float32(np.inf)] + [np.float32(1.0)] * 6
    # stereo counts 10 (mThDepth itself, the neighbour below, -0, NaN, six plain) with 9 redundant:
    # kept; mono counts all 13 with 12 redundant: culled.  The one that is not redundant sits on mThDepth
    w.keyframe("Z", 13, depth=[float(x) for x in z], th=float(th))
    w.redundant_points("Z", "zq_", 1, 0, first=0)
    w.redundant_points("Z", "z_", 12, 12, first=1)
    s = w.script()
    s.append(("update_batch", w.helpers + w.kfs))
    mono = bool(v % 2)
    s.append(("setordered", "H3", [(n, 50 - i) for i, n in enumerate(["B9", "D18", "E0", "Z"])]))
    s.append(("cullkfs", "H3", ["D2"], "D2", mono))           # redundant, but the map's first keyframe
    s.append(("cullkfs", "H3", None, None, mono))             # nothing culled but perhaps Z
    s.append(("cullkfs", "H3", ["B9", "D18", "E0", "Z", "D2"], None, not mono))
    s.append(("cullkfs", "H3", [], None, mono))
    s.append(("noterase", "C", True))
    s.append(("cullkfs", "H3", ["H0", "C", "B9", "C"], "H0", mono))   # deferred twice
    s.append(("seterase", "C", True))
    s.append(("seterase", "C", False))
    if v % 3 == 0:
        s.append(("cullkfs", "H3", ["B9", "A", "F", "D18", "A2", "G", "Z"], "B9", mono))
    elif v % 3 == 1:
        s.append(("cullkfs", "H3", ["F", "G", "A2", "A", "F", "G"], None, mono))
    else:
        s.append(("cullkfs", "H3", ["A2", "G", "A", "F", "A", "Z"], "Z", mono))
    s.append(("cullkfs", "H3", w.kfs, None, False))
    s.append(("mpbad", ["b9_9"], True))                       # the one that was not redundant: 9 of 9
    s.append(("cullkfs", "H3", ["B9"], None, mono))
    s.append(("unobs", [("b9_0", "H0")]))
    s.append(("obs", [("b9_0", "H0")]))
    s.append(("cullkfs", "H3", ["D18"], None, mono))          # an index is unknown: refused
    return s


CASES = {"observations": case_observations, "badflag": case_badflag, "cullpoints": case_cullpoints,
         "counters": case_counters, "kfbadflag": case_kfbadflag, "cullkfs": case_cullkfs}
VARIANTS = range(6)


def built_scripts():
    for name, fn in CASES.items():
        for v in VARIANTS:
            yield f"{name}-{v}", fn(v)


def seeded_script(seed, nkf=7, npts=60, n_ops=14):
    """A random map (entries overwritten after being observed, observations without an index,
    right coordinates) and a random walk of the culling operations."""
    r = random.Random(seed)
    s = []
    pts = [f"p{i}" for i in range(npts)]
    s.append(("points", pts))
    kfs = [f"k{i}" for i in range(nkf)]
    keys = r.sample(range(1, 1 << 16), nkf)
    slots = {}
    for i, n in enumerate(kfs):
        mps = [r.choice(pts) if r.random() < 0.85 else None for _ in range(r.randrange(20, 40))]
        slots[n] = len(mps)
        s.append(("kf", n, BASE + 16 * keys[i], mps))
        s.append(("features", n, [r.randrange(8) for _ in mps], [r.choice((-1.0, 3.5)) for _ in mps],
                  None, 40.0))
        s.append(("obsidx", [(p, n, j) for j, p in enumerate(mps) if p is not None and r.random() < 0.9]))
    s.append(("obs", [(r.choice(pts), r.choice(kfs)) for _ in range(4)]))
    s.append(("counters", pts, None, [r.randrange(0, 9) for _ in pts], [r.randrange(0, 20) for _ in pts],
              [r.randrange(0, 6) for _ in pts]))
    for _ in range(n_ops):
        c = r.random()
        if c < 0.2:
            k = r.choice(kfs)
            s.append(("obsidx", [(r.choice(pts), k, r.randrange(slots[k])) for _ in range(5)]))
        elif c < 0.35:
            s.append(("eraseobs", r.choice(pts), r.choice(kfs)))
        elif c < 0.45:
            s.append(("mpbadflag", r.sample(pts, 3)))
        elif c < 0.55:
            s.append(("inc", r.choice(("found", "visible")), [r.choice(pts) for _ in range(6)],
                      r.choice((None, [r.randrange(4) for _ in range(6)]))))
        elif c < 0.65:
            s.append(("tracked", r.choice(kfs), r.randrange(5)))
        elif c < 0.7:
            k = r.choice(kfs)
            s.append(("kfpoints", k, 0, [r.choice(pts + [None]) for _ in range(4)]))
        else:
            s.append(("cullpoints", [r.choice(pts) for _ in range(r.choice((1, 5, 20, 70)))],
                      r.randrange(0, 9), r.random() < 0.5))
    return s


def seeded_kf_script(seed, nkf=9, npts=44, n_ops=6):
    """A dense random map (most points seen by five or six keyframes at octaves 0..2, a few held
    twice or held without being listed, stereo depths around mThDepth), its graph and tree from
    UpdateConnections, and a random walk of KeyFrameCulling over covisibility lists and explicit
    lists, SetBadFlag, SetNotErase / SetErase and single erases."""
    r = random.Random(seed)
    s = []
    pts = [f"p{i}" for i in range(npts)]
    s.append(("points", pts))
    kfs = [f"k{i}" for i in range(nkf)]
    keys = r.sample(range(1, 1 << 16), nkf)
    for i, n in enumerate(kfs):
        mps = r.sample(pts, r.randrange(30, 40))
        mps[r.randrange(len(mps))] = r.choice(mps)                       # held twice
        mps = [p if r.random() < 0.95 else None for p in mps]
        s.append(("kf", n, BASE + 16 * keys[i], mps))
        s.append(("features", n, [r.choice((0, 0, 0, 1, 2)) for _ in mps], [r.choice((-1.0, 3.5)) for _ in mps],
                  [r.choice((0.5, 1.0, 2.0, 2.0, 3.0, 3.0, 2.5, 3.5, -1.0)) for _ in mps], 3.0))
        s.append(("obsidx", [(p, n, j) for j, p in enumerate(mps) if p is not None and r.random() < 0.97]))
    s.append(("update_batch", kfs))
    s.append(("mpbad", r.sample(pts, 2), True))
    for _ in range(n_ops):
        c = r.random()
        if c < 0.45:
            s.append(("cullkfs", r.choice(kfs), None, r.choice(kfs + [None]), r.random() < 0.5))
        elif c < 0.6:
            s.append(("cullkfs", r.choice(kfs), [r.choice(kfs) for _ in range(r.choice((1, 3, 6, 12)))],
                      r.choice(kfs + [None]), r.random() < 0.5))
        elif c < 0.7:
            s.append(("kfbadflag", r.choice(kfs), r.random() < 0.1))
        elif c < 0.8:
            s.append(("noterase", r.choice(kfs), r.random() < 0.7))
        elif c < 0.9:
            s.append(("seterase", r.choice(kfs), r.random() < 0.3))
        else:
            s.append(("eraseobs", r.choice(pts), r.choice(kfs)))
    return s


# ---- the shapes at which a kernel can break (tests/test_gpu_culling.py) ------------------------
def script_observation_rows(sizes=(0, 1, 2, 3, 4, 63, 64, 65, 200), v=1):
    """One point per observation-row size (every observer holds it at another slot), every point
    set bad in one call; then the same rows culled by MapPointCulling."""
    s = []
    nkf = max(sizes)
    names = [f"K{i}" for i in range(nkf)]
    pts = [f"r{n}" for n in sizes] + [f"c{n}" for n in sizes]
    s.append(("points", pts))
    for i, (n, key) in enumerate(zip(names, keys_for(nkf, v))):
        s.append(("kf", n, key, [pts[(i + j) % len(pts)] for j in range(2 * len(pts))]))
        s.append(("features", n, None, [1.0 if (i + j) % 5 == 0 else -1.0 for j in range(2 * len(pts))], None, 0.0))
    obs = []
    for q, n in enumerate(sizes):
        for i in range(n):
            k = (3 * i + q) % nkf if n < nkf else i
            for p in (q, q + len(sizes)):
                obs.append((pts[p], names[k], (p - k) % len(pts) + (len(pts) if i % 2 else 0)))
    s.append(("obsidx", obs))
    s.append(("mpbadflag", pts[:len(sizes)]))
    s.append(("counters", pts[len(sizes):], None, [0] * len(sizes), [1] * len(sizes), None))
    s.append(("cullpoints", pts[len(sizes):], 0, False))
    return s


def script_keyframe_slots(sizes=(0, 1, 63, 64, 65, 1024, 1025, 8192), v=0):
    """Keyframes of every slot count: TrackedMapPoints over them, features set and read back, and a
    point held at the last slot of each set bad."""
    s = []
    npts = 64
    pts = [f"p{i}" for i in range(npts)] + [f"last{n}" for n in sizes]
    s.append(("points", pts))
    names = [f"S{n}" for n in sizes]
    for n, name, key in zip(sizes, names, keys_for(len(sizes), v)):
        mps = [pts[(7 * j) % npts] if j % 9 else None for j in range(n)]
        if n:
            mps[-1] = f"last{n}"
        s.append(("kf", name, key, mps))
        s.append(("features", name, [j % 128 for j in range(n)], [float(j % 3) - 1.0 for j in range(n)],
                  [float(j) / 7 for j in range(n)], 3.0 * n))
        if n:
            s.append(("obsidx", [(f"last{n}", name, n - 1)] +
                      [(p, name, j) for j, p in enumerate(mps[:npts]) if p is not None and p not in mps[:j]]))
    s.append(("mpbad", pts[3:6], True))
    for name in names:
        for mo in (0, 1, 2, 4):
            s.append(("tracked", name, mo))
    s.append(("mpbadflag", [f"last{n}" for n in sizes]))
    s.append(("tracked", names[-1], 1))
    return s


def script_cull_list(n, v=0):
    """A list of n entries over 40 points (so points repeat from n = 41 on), one of each branch in
    rotation."""
    s, names, pts = _map(v, 3, 40)
    s.append(("obsidx", [(p, k, j) for j, p in enumerate(pts) for k in names]))
    s.append(("counters", pts, [(2, 3, 4, 9)[j % 4] for j in range(40)], [(1, 5, 0, 2)[j % 4] for j in range(40)],
              [(5, 5, 0, 9)[(j // 4) % 4] for j in range(40)], [j % 5 for j in range(40)]))
    s.append(("mpbad", pts[::11], True))
    r = random.Random(n)
    s.append(("cullpoints", [pts[r.randrange(40)] for _ in range(n)], 4, bool(v % 2)))
    return s


def script_kf_list(n, share=True, octave=1, v=0):
    """n listed keyframes L0.. of 20 slots, two helpers and the current keyframe, whose ordered list
    they are.  share: point set P_i is seen by L_i, L_i+1 and the helpers, so a cull takes the
    third observer from its successor and every second keyframe goes; else every keyframe has its
    own points and three helpers: all go (helpers at `octave` against the keyframes' 1; 3: none)."""
    helpers = ["H0", "H1", "H2"]
    names = helpers + ["Cur"] + [f"L{i}" for i in range(n)]
    held = {h: [] for h in helpers}
    held.update({x: [None] * 20 for x in names[3:]})
    pts, obs = [], []
    for i in range(n):
        for j in range(10):
            p = f"s{i}_{j}"
            pts.append(p)
            seen = [(f"L{i}", j)] + ([(f"L{i + 1}", 10 + j)] if share and i + 1 < n else [])
            for h in helpers[:2 if share else 3]:
                held[h].append(p)
                seen.append((h, len(held[h]) - 1))
            for k, x in seen:
                if not k.startswith("H"):
                    held[k][x] = p
                obs.append((p, k, x))
    s = [("points", pts)]
    for name, key in zip(names, keys_for(len(names), v)):
        s.append(("kf", name, key, held[name]))
        s.append(("features", name, [octave if name in helpers else 1] * len(held[name]), None, None, 0.0))
    s.append(("obsidx", obs))
    s.append(("update_batch", names[:40]))
    s.append(("setordered", "Cur", [(f"L{i}", n - i) for i in range(n)]))
    s.append(("cullkfs", "Cur", None, None, True))
    return s


def script_kf_children(nc, v=0):
    """Keyframe X with a parent P and nc children: every third is connected to P, the next one to
    the child before it only (a candidate once that one has left), the third to nobody."""
    names = ["Z", "P", "X"] + [f"c{i}" for i in range(nc)]
    pts = [f"x{j}" for j in range(6)]
    s = [("points", pts)]
    for name, key in zip(names, keys_for(len(names), v)):
        s.append(("kf", name, key, pts if name in ("X", "P", "Z", "c0") else []))
    s.append(("features", "X", [0] * 6, [1.0, -1.0] * 3, None, 0.0))
    s.append(("obsidx", [(p, k, j) for j, p in enumerate(pts) for k in names[:3 + min(nc, 1)] if (j + len(k)) % 3]))
    s.append(("parent", "X", "P"))
    s.append(("children", "P", ["X"]))
    s.append(("children", "X", names[3:]))
    for i in range(nc):
        c = f"c{i}"
        s.append(("parent", c, "X"))
        if i % 3 == 0:
            conn = [("P", 5 + i % 4), ("X", 40)]
        elif i % 3 == 1:
            conn = [(f"c{i - 1}", 7), ("X", 40)]
        else:
            conn = [("X", 40), ("Z", 3)]
        s.append(("setconn", c, conn))
        s.append(("best", c))
    s.append(("setconn", "X", [(f"c{i}", 40) for i in range(nc)]))
    s.append(("kfbadflag", "X"))
    return s


def script_kf_big(v=0):
    """An 8,192-slot keyframe G among three more that hold the same points at the same slots: 5,000
    points seen by all four, the rest by three, so that G's SetBadFlag sets 3,192 points bad."""
    n = K.L.MAX_KF_SLOTS
    pts = [f"q{i}" for i in range(n)]
    s = [("points", pts)]
    names = ["A", "B", "C", "G"]
    for name, key in zip(names, keys_for(4, v)):
        s.append(("kf", name, key, pts[:-50] + [pts[0]] * 50 if name == "G" else pts))
        s.append(("features", name, [i % 2 for i in range(n)], [1.0 if i % 7 == 0 else -1.0 for i in range(n)],
                  None, 0.0))
    s.append(("obsidx", [(p, k, i) for i, p in enumerate(pts) for k in names if k != "C" or i < 5000]))
    s.append(("counters", pts[6000:6100], [9] * 100, None, None, None))
    s.append(("cullkfs", "A", ["G", "A"], None, True))
    s.append(("kfbadflag", "G"))
    return s
