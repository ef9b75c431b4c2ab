"""KeyFrameDatabase and ORBVocabulary::score restated in plain Python from the reference's lines
(KeyFrameDatabase.cc:115-389, ScoringObject.cpp:23-311, KeyFrame.h:166-171), with real per-word
lists, the six per-keyframe state fields, branch counters and single-decision mutants; and the
built cases (scripts of adds, erases and queries) that tests/test_kfdb.py proves non-trivial and
tests/test_gpu_kfdb.py runs against the library.

A script is a list of operations on keyframes named by strings:
    ("add", name, ids, vals)            KeyFrameDatabase::add
    ("erase", name)                     KeyFrameDatabase::erase
    ("clear",)
    ("covis", name, [names or None])    GetBestCovisibilityKeyFrames(10); None = not in the database
    ("scores", name, loop, reloc)       archived mLoopScore / mRelocScore
    ("loop", qid, ids, vals, [connected names], min_score)
    ("reloc", qid, ids, vals)
A query's answer is (candidate names in order, h18 flag, state of every keyframe).
"""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np

F32 = np.float32
SCORINGS = (0, 1, 2, 4, 5)  # L1, L2, chi-square, Bhattacharyya, dot product (3 = KL: unsupported)

MUTANTS = ("words_ge", "minscore_gt", "retain_ge", "best_ge", "double_acc", "key_swapped",
           "slot_for_seq", "loop_no_words_test", "reloc_words_test", "reverse_sum",
           "conn_keeps_words", "h19_reset", "below_min_no_feed", "conn_listed",
           "score_only_if_kept")


def _bump(stats, key):
    if stats is not None:
        stats[key] = stats.get(key, 0) + 1


def fma(a: float, b: float, c: float) -> float:
    """a * b + c rounded once (Fraction -> float rounds to nearest even)."""
    if any(math.isinf(x) or math.isnan(x) for x in (a, b, c)):
        return a * b + c
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def common(ids1, ids2):
    """Index pairs of the common words in ascending word order — what the merge walk with
    lower_bound visits (ScoringObject.cpp:34-59)."""
    i1 = np.asarray(ids1, np.int64)
    i2 = np.asarray(ids2, np.int64)
    _, a, b = np.intersect1d(i1, i2, assume_unique=True, return_indices=True)
    return list(zip(a.tolist(), b.tolist()))


def score(scoring, ids1, vals1, ids2, vals2, fused=True, order="forward"):
    """ORBVocabulary::score(v1, v2).  fused: `score += vi * wi` contracted to one fma, as GCC -O3
    -march=native builds the L2 and dot-product loops (:91, :290).  order: 'forward' is the
    reference's; 'reverse' and 'pairwise' are the wrong summation orders the tests tell apart."""
    assert scoring in SCORINGS
    terms = []
    for a, b in common(ids1, ids2):
        vi, wi = float(vals1[a]), float(vals2[b])
        if scoring == 0:
            terms.append((abs(vi - wi) - abs(vi) - abs(wi), None))       # :41
        elif scoring == 2:
            if vi + wi != 0.0:                                              # :148
                terms.append((vi * wi / (vi + wi), None))
        elif scoring == 4:
            terms.append((math.sqrt(vi * wi) if vi * wi >= 0 else float("nan"), None))  # :245
        else:
            terms.append((vi * wi, (vi, wi)))                               # :91, :290
    if order == "reverse":
        terms = terms[::-1]
    if order == "pairwise":
        vals = [t for t, _ in terms]
        while len(vals) > 1:
            vals = [vals[i] + vals[i + 1] if i + 1 < len(vals) else vals[i]
                    for i in range(0, len(vals), 2)]
        s = vals[0] if vals else 0.0
    else:
        s = 0.0
        for t, prod in terms:
            s = fma(prod[0], prod[1], s) if (fused and prod is not None) else s + t
    if scoring == 0:
        s = -s / 2.0                                                        # :65
    elif scoring == 1:
        s = 1.0 if s >= 1 else 1.0 - math.sqrt(1.0 - s)                     # :114-117
    elif scoring == 2:
        s = 2. * s                                                          # :167
    return s


class KF:
    """The KeyFrame members the database touches (KeyFrame.h:166-171; KeyFrame.cc:35, :64 set the
    four integers to 0 and leave the two scores uninitialised: None here)."""

    def __init__(self, name, ids, vals, slot, seq):
        self.name, self.slot, self.seq = name, slot, seq
        self.ids = np.asarray(ids, np.int32)
        self.vals = np.asarray(vals, np.float64)
        self.loop_query = 0
        self.loop_words = 0
        self.loop_score = None
        self.reloc_query = 0
        self.reloc_words = 0
        self.reloc_score = None
        self.neigh = []
        self.first = None  # first common word of the current walk

    def state(self):
        bits = lambda x: None if x is None else int(np.array(x, F32).view(np.uint32))
        return (self.loop_query, self.loop_words, bits(self.loop_score), self.reloc_query,
                self.reloc_words, bits(self.reloc_score))


class DB:
    def __init__(self, scoring=0, fused=True, mutant=None, stats=None):
        assert mutant is None or mutant in MUTANTS
        self.scoring, self.fused, self.mutant, self.stats = scoring, fused, mutant, stats
        self.inv = {}            # mvInvertedFile: word -> list of KF
        self.kfs = {}            # name -> KF
        self.free, self.hi, self.next_seq = [], 0, 0

    # -- KeyFrameDatabase::add (:115-121); slots as the library hands them out (the most recently
    #    freed first), so that the slot_for_seq mutant means something
    def add(self, name, ids, vals):
        assert name not in self.kfs
        if self.free:
            slot = self.free.pop()
        else:
            slot = self.hi
            self.hi += 1
        kf = KF(name, ids, vals, slot, self.next_seq)
        self.next_seq += 1
        self.kfs[name] = kf
        for w in kf.ids.tolist():
            self.inv.setdefault(w, []).append(kf)
        return kf

    # -- KeyFrameDatabase::erase (:123-142); the library also drops the keyframe from every
    #    covisibility list (a neighbour entry never names a recycled slot)
    def erase(self, name):
        kf = self.kfs.pop(name)
        for w in kf.ids.tolist():
            self.inv[w].remove(kf)
        for o in self.kfs.values():
            o.neigh = [None if n is kf else n for n in o.neigh]
        self.free.append(kf.slot)

    def clear(self):                                                        # :144-148
        self.inv, self.kfs, self.free, self.hi = {}, {}, [], 0

    def covis(self, name, names):
        assert len(names) <= 10
        self.kfs[name].neigh = [None if n is None else self.kfs[n] for n in names]

    def scores(self, name, loop, reloc):
        self.kfs[name].loop_score, self.kfs[name].reloc_score = F32(loop), F32(reloc)

    def _score(self, ids, vals, kf):
        order = "reverse" if self.mutant == "reverse_sum" else "forward"
        return score(self.scoring, ids, vals, kf.ids, kf.vals, self.fused, order)

    def _sharing_order(self, sharing):
        """lKFsSharingWords is in first-encounter order of the walk; that order is the key (first
        common word, add sequence).  The mutants sort by a wrong key."""
        natural = sorted(sharing, key=lambda k: (k.first, k.seq))
        assert [k.name for k in natural] == [k.name for k in sharing]
        if self.mutant == "key_swapped":
            return sorted(sharing, key=lambda k: (k.seq, k.first))
        if self.mutant == "slot_for_seq":
            return sorted(sharing, key=lambda k: (k.first, k.slot))
        return sharing

    def _tail(self, loop, qid, scored, min_common, best_acc):
        """:223-271 / :342-388 -> (candidate names, h18)."""
        st, mu = self.stats, self.mutant
        h18 = False
        acc_list = []
        for si, kf in scored:
            best_score = si
            acc = float(si) if mu == "double_acc" else si
            best_kf = kf
            for n in kf.neigh[:10]:
                if n is None:
                    _bump(st, "neigh_absent")
                    continue
                if loop:
                    ok = n.loop_query == qid and (mu == "loop_no_words_test" or n.loop_words > min_common)  # :234
                    if ok and mu == "below_min_no_feed" and not (n.loop_score is not None and n.loop_score >= self._min_score):
                        ok = False
                else:
                    ok = n.reloc_query == qid                                # :353
                    if mu == "reloc_words_test":
                        ok = ok and n.reloc_words > min_common
                if not ok:
                    _bump(st, "neigh_skipped")
                    continue
                v = n.loop_score if loop else n.reloc_score
                if v is None:                                               # H18
                    _bump(st, "h18")
                    h18 = True
                    v = F32(0.0)
                elif n not in self._scored_now:
                    _bump(st, "neigh_stale_score")
                _bump(st, "neigh_counted")
                acc = acc + (float(v) if mu == "double_acc" else v)       # :236 / :356
                if (v >= best_score) if mu == "best_ge" else (v > best_score):
                    _bump(st, "best_moves")
                    best_kf, best_score = n, v
            acc_list.append((acc, best_kf))
            if acc > best_acc:
                best_acc = acc
        retain = (0.75 * best_acc) if mu == "double_acc" else F32(0.75) * F32(best_acc)  # :251 / :370
        out, seen = [], set()
        for acc, kf in acc_list:
            if acc == retain:
                _bump(st, "retain_equal")
            if (acc >= retain) if mu == "retain_ge" else (acc > retain):    # :259 / :377
                _bump(st, "retain_pass")
                if kf.name in seen:
                    _bump(st, "duplicate_best")
                    continue
                seen.add(kf.name)
                out.append(kf.name)
            else:
                _bump(st, "retain_fail")
        return out, h18

    def _min_common(self, sharing, words_of):
        max_common = 0
        for kf in sharing:                                                  # :188-193 / :308-313
            max_common = max(max_common, words_of(kf))
        return int(F32(max_common) * F32(0.8))                              # :195 / :315

    def detect_loop(self, qid, ids, vals, connected, min_score):
        """KeyFrameDatabase::DetectLoopCandidates (:151-272)."""
        st, mu = self.stats, self.mutant
        conn = {self.kfs[n] for n in connected if n in self.kfs}
        min_score = F32(min_score)
        self._min_score = min_score
        sharing, seen = [], set()
        for w in np.asarray(ids).tolist():                                  # :161
            for kf in self.inv.get(w, []):                                  # :165
                fresh = kf.name not in seen
                seen.add(kf.name)
                if kf.loop_query != qid or (mu == "h19_reset" and fresh):   # :168
                    if not (mu == "conn_keeps_words" and not fresh):
                        kf.loop_words = 0                                   # :170
                    if kf not in conn or mu == "conn_listed":               # :171
                        _bump(st, "walk_first")
                        kf.loop_query = qid
                        kf.first = w
                        sharing.append(kf)
                    else:
                        _bump(st, "walk_connected")
                elif kf in sharing:
                    _bump(st, "walk_again")
                else:
                    _bump(st, "walk_collision")                             # H19
                kf.loop_words += 1                                          # :177
        if not sharing:                                                     # :182
            _bump(st, "exit_no_sharing")
            return [], False
        sharing = self._sharing_order(sharing)
        min_common = self._min_common(sharing, lambda k: k.loop_words)
        scored = []
        self._scored_now = set()
        for kf in sharing:                                                  # :200
            if kf.loop_words == min_common:
                _bump(st, "words_equal_min")
            if (kf.loop_words >= min_common) if mu == "words_ge" else (kf.loop_words > min_common):  # :204
                _bump(st, "words_pass")
                si = F32(self._score(ids, vals, kf))                        # :208
                if mu != "score_only_if_kept" or si >= min_score:
                    kf.loop_score = si                                      # :210
                self._scored_now.add(kf)
                if si == min_score:
                    _bump(st, "score_equal_min")
                if (si > min_score) if mu == "minscore_gt" else (si >= min_score):  # :211
                    _bump(st, "score_pass")
                    scored.append((si, kf))
                else:
                    _bump(st, "score_fail")
            else:
                _bump(st, "words_fail")
        if not scored:                                                      # :216
            _bump(st, "exit_no_scored")
            return [], False
        return self._tail(True, qid, scored, min_common, min_score)         # :220

    def detect_reloc(self, qid, ids, vals):
        """KeyFrameDatabase::DetectRelocalizationCandidates (:274-389)."""
        st, mu = self.stats, self.mutant
        sharing, seen = [], set()
        for w in np.asarray(ids).tolist():                                  # :282
            for kf in self.inv.get(w, []):                                  # :287
                fresh = kf.name not in seen
                seen.add(kf.name)
                if kf.reloc_query != qid or (mu == "h19_reset" and fresh):  # :292
                    _bump(st, "walk_first")
                    kf.reloc_words = 0
                    kf.reloc_query = qid
                    kf.first = w
                    sharing.append(kf)
                elif kf in sharing:
                    _bump(st, "walk_again")
                else:
                    _bump(st, "walk_collision")                             # H19
                kf.reloc_words += 1                                         # :300
        if not sharing:                                                     # :304
            _bump(st, "exit_no_sharing")
            return [], False
        sharing = self._sharing_order(sharing)
        min_common = self._min_common(sharing, lambda k: k.reloc_words)
        scored = []
        self._scored_now = set()
        for kf in sharing:                                                  # :322
            if kf.reloc_words == min_common:
                _bump(st, "words_equal_min")
            if (kf.reloc_words >= min_common) if mu == "words_ge" else (kf.reloc_words > min_common):  # :326
                _bump(st, "words_pass")
                si = F32(self._score(ids, vals, kf))                        # :329
                kf.reloc_score = si
                self._scored_now.add(kf)
                scored.append((si, kf))
            else:
                _bump(st, "words_fail")
        if not scored:                                                      # :335 (unreachable: the
            return [], False                                                # keyframe of maxCommonWords passes)
        return self._tail(False, qid, scored, min_common, F32(0))           # :339

    def states(self):
        return {n: k.state() for n, k in self.kfs.items()}


def run_script(script, scoring=0, fused=True, mutant=None, stats=None):
    """-> the answers of the script's queries: (candidates, h18, states)."""
    db = DB(scoring, fused, mutant, stats)
    out = []
    for op in script:
        if op[0] == "add":
            db.add(*op[1:])
        elif op[0] == "erase":
            db.erase(op[1])
        elif op[0] == "clear":
            db.clear()
        elif op[0] == "covis":
            db.covis(op[1], op[2])
        elif op[0] == "scores":
            db.scores(*op[1:])
        elif op[0] == "loop":
            c, h = db.detect_loop(*op[1:])
            out.append((c, h, db.states()))
        elif op[0] == "reloc":
            c, h = db.detect_reloc(*op[1:])
            out.append((c, h, db.states()))
        else:
            raise ValueError(op[0])
    return out


# ==== built cases ===============================================================================
# L1 scoring with dyadic values: the score of a keyframe that shares c words at value w with a
# query of value q is c * min(w, q) exactly, so thresholds can be met with equality.

NQ = 20
QV = 1.0 / 32


def _query(v):
    base = 50 + 7 * v
    return base + np.arange(NQ, dtype=np.int32), np.full(NQ, QV)


def _kf(v, idx, val=QV, private=0):
    """A BowVector sharing the query words `idx` (positions in the query) at value val, plus
    `private` words of its own above the query's range."""
    base = 50 + 7 * v
    ids = [base + i for i in idx] + [base + 1000 + 13 * private + j for j in range(3)]
    return np.array(sorted(ids), np.int32), np.full(len(ids), val)


def case_thresholds(v):
    """Word-count ties, words == minCommonWords (excluded), si == minScore (kept), accScore ==
    minScoreToRetain (dropped), order by first common word against add order and by sequence
    within a word; reloc then loop with the same id (H19 does not apply: separate fields)."""
    q = _query(v)
    s = [("add", "E", *_kf(v, [19], private=1)),
         ("add", "B", *_kf(v, range(5, 15), private=2)),      # 10 words, first word 5
         ("add", "D", *_kf(v, range(1, 10), private=3)),      # 9 words
         ("add", "C", *_kf(v, range(2, 10), private=4)),      # 8 == minCommonWords: excluded
         ("add", "G", *_kf(v, range(3, 13), val=3.0 / 128, private=5)),  # 30/128 == 0.75 * 10/32
         ("add", "A2", *_kf(v, range(0, 10), private=6)),     # same first word as A, added first
         ("add", "A", *_kf(v, range(0, 10), private=7)),
         ("reloc", 7 + v, *q),
         ("loop", 7 + v, *q, [], 9.0 / 32),                   # D's score == minScore: kept
         ("loop", 100 + v, *q, [], 9.5 / 32)]                 # D below
    return s


def case_covisibility(v):
    """A neighbour outscoring its keyframe, two entries naming the same best keyframe, a full list
    with an absent neighbour in the tenth place, a connected keyframe with many common words, and
    a keyframe below minScore that still feeds its neighbour's accumulated score."""
    q = _query(v)
    s = [("add", "P", *_kf(v, range(0, 10), private=1)),               # 10/32
         ("add", "K", *_kf(v, range(1, 10), private=2)),               # 9/32, neighbour P outscores
         ("add", "L", *_kf(v, range(2, 12), val=1.0 / 128, private=3)),  # 10/128: below minScore
         ("add", "M", *_kf(v, range(4, 13), private=4)),               # 9/32 + L's 10/128
         ("add", "W", *_kf(v, range(6, 15), val=1.0 / 40, private=5)),   # 9/40: retained only by the margin
         ("add", "CN", *_kf(v, range(0, 16), private=6)),              # connected, 16 common words
         ("add", "Z", *_kf(v, [], private=7))]                         # shares nothing
    s += [("add", "f%d" % i, *_kf(v, [], private=10 + i)) for i in range(8)]
    s += [("covis", "K", ["P"]),
          ("covis", "M", ["Z", "L"] + ["f%d" % i for i in range(7)] + [None]),
          ("covis", "W", ["f%d" % i for i in range(8)] + ["Z", None]),
          ("covis", "P", ["K", "CN"]),
          ("loop", 30 + v, *q, ["CN", "Z"], 8.0 / 32),
          ("reloc", 30 + v, *q),
          ("loop", 60 + v, *q, ["CN"], 9.0 / 32)]
    return s


def case_stale_scores(v):
    """A relocalisation neighbour whose score comes from an earlier query (:353 tests the id
    only); the same without the earlier query (H18: the reference reads an uninitialised float);
    archived scores; and the loop form's neighbour test with mnLoopWords."""
    q1 = _query(v)
    base = 50 + 7 * v
    q2 = (base + 200 + np.arange(NQ, dtype=np.int32), np.full(NQ, QV))

    def kf2(idx, extra=(), val=QV):
        ids = sorted([base + 200 + i for i in idx] + [base + i for i in extra])
        return np.array(ids, np.int32), np.full(len(ids), val)
    s = [("add", "X", *kf2([0], extra=range(0, 10))),     # 10 words of q1, 1 word of q2
         ("add", "Y", *kf2(range(0, 10))),
         ("add", "Z", *kf2(range(1, 11), val=1.0 / 40)),
         ("add", "U", *kf2([5], extra=[19])),             # never scored: H18 when counted
         ("covis", "Y", ["X"]),
         ("reloc", 11 + v, *q1),                          # X scored 10/32
         ("reloc", 12 + v, *q2),                          # X listed, not scored: stale 10/32 feeds Y
         ("loop", 11 + v, *q1, [], 1.0 / 32),
         ("loop", 12 + v, *q2, [], 1.0 / 32),             # X's mnLoopWords 1 fails the loop test
         ("covis", "Z", ["U"]),
         ("reloc", 13 + v, *q2),                          # U listed, never scored: H18
         ("loop", 13 + v, *q2, [], 1.0 / 32),
         ("scores", "U", 2.0, 3.0),
         ("reloc", 14 + v, *q2),                          # the archived mRelocScore counts
         ("loop", 14 + v, *q2, [], 1.0 / 32)]
    return s


def case_collisions(v):
    """H19: query id 0 against fresh keyframes (mnLoopQuery / mnRelocQuery start at 0), the same
    id queried twice (a keyframe's words go on from the stale count and its stale score feeds a
    neighbour), and a collision that reads a score never written (H18 in the loop form)."""
    q = _query(v)
    base = 50 + 7 * v
    qa = (base + np.arange(5, dtype=np.int32), np.full(5, QV))
    s = [("add", "A", *_kf(v, range(0, 10), private=1)),
         ("add", "B", *_kf(v, range(3, 12), private=2)),
         ("add", "C", *_kf(v, range(10, 19), private=3)),
         ("covis", "C", ["A", "B"]),
         ("covis", "B", ["A"]),
         ("reloc", 0, *q),                                # every keyframe collides: no candidates
         ("loop", 0, *q, [], 1.0 / 32),
         ("loop", 0, *q, ["B"], 1.0 / 32),                # words go on: 2c
         ("reloc", 5 + v, *qa),                           # touches A and B only
         ("reloc", 5 + v, *q),                            # A, B collide; C listed, reads their scores
         ("loop", 5 + v, *qa, [], 1.0 / 32),
         ("loop", 5 + v, *q, [], 1.0 / 32),
         ("add", "D", *_kf(v, range(8, 18), private=4)),
         ("covis", "D", ["A", "C"]),
         ("loop", 0, *q, [], 1.0 / 32)]                   # D fresh with id 0: collides, nothing listed
    return s


def case_erase_reuse(v):
    """Erase, then add into the freed slot, with a covisibility list that named the erased
    keyframe; slot order and add order differ afterwards."""
    q = _query(v)
    s = [("add", "A", *_kf(v, range(0, 9), private=1)),
         ("add", "B", *_kf(v, range(0, 10), private=2)),
         ("add", "C", *_kf(v, range(0, 9), val=1.0 / 40, private=3)),
         ("add", "E", *_kf(v, range(0, 9), val=1.0 / 36, private=5)),
         ("covis", "C", ["B"]),
         ("covis", "A", ["B"]),
         ("reloc", 21 + v, *q),
         ("erase", "B"),
         ("add", "D", *_kf(v, range(0, 10), private=4)),  # takes B's slot, last in add order
         ("reloc", 22 + v, *q),                           # C's list no longer names that slot
         ("loop", 22 + v, *q, [], 1.0 / 64),
         ("erase", "A"),
         ("erase", "C"),
         ("add", "F", *_kf(v, range(0, 10), private=6)),  # C's slot
         ("add", "G", *_kf(v, range(0, 10), private=7)),  # A's slot
         ("covis", "G", ["F", None, "D"]),
         ("reloc", 23 + v, *q),
         ("loop", 23 + v, *q, ["E"], 1.0 / 64),
         ("clear",),
         ("reloc", 24 + v, *q),
         ("add", "H", *_kf(v, range(0, 10), private=8)),
         ("reloc", 25 + v, *q)]
    return s


def case_all_below(v):
    """The loop form's second early return (:216): keyframes share enough words and are scored,
    every score is below minScore, nothing is listed — and mnLoopQuery, mnLoopWords and mLoopScore
    stay written.  The next query with the same id finds them colliding (H19) and reads those
    scores through a neighbour list; a query with another id starts afresh."""
    q = _query(v)
    s = [("add", "A", *_kf(v, range(0, 10), val=1.0 / 128, private=1)),   # 10/128
         ("add", "B", *_kf(v, range(2, 11), val=1.0 / 64, private=2)),    # 9/64
         ("add", "C", *_kf(v, range(0, 5), private=3)),                   # too few words: unscored
         ("add", "D", *_kf(v, range(5, 15), private=4)),                  # connected
         ("covis", "B", ["A", "C"]),
         ("loop", 70 + v, *q, ["D"], 0.25),                               # all below: exit at :216
         ("loop", 70 + v, *q, [], 0.25),                                  # A, B, C collide; D listed
         ("add", "E", *_kf(v, range(1, 11), val=1.0 / 64, private=5)),
         ("covis", "E", ["B", "A"]),
         ("loop", 70 + v, *q, ["D"], 0.125),                              # E listed, feeds on stale scores
         ("loop", 170 + v, *q, ["D"], 0.5),                               # afresh, all below again
         ("loop", 270 + v, *q, ["D"], 9.0 / 64)]                          # B and E at minScore exactly
    return s


def case_rounding(v):
    """Dot-product scoring with a query of ones, so a keyframe's score is the sum of its values in
    word order.  Float against double accumulation: BEST's accumulated score 1 + 1.25 * 2^-24
    rounds to 1 + 2^-23 in float, minScoreToRetain to 0.75 + 2 ulp, and R at 0.75 + 1 ulp is
    dropped (kept if either were double).  Summation order: S's terms 1, 2^60, -2^60 give 0 in
    word order and 1 in reverse, across minScore."""
    base = 50 + 7 * v
    ids = base + np.arange(4, dtype=np.int32)
    q = (ids, np.ones(4))
    u = 2.0 ** -24
    s = [("add", "R", ids, np.array([u, 0.25, 0.25, 0.25])),
         ("add", "N", ids, np.full(4, 1.25 * u / 4)),
         ("add", "BEST", ids, np.full(4, 0.25)),
         ("add", "S", ids, np.array([1.0, 2.0 ** 60, -2.0 ** 60, 0.0])),
         ("covis", "BEST", ["N"]),
         ("reloc", 40 + v, *q),
         ("loop", 40 + v, *q, [], 0.5)]
    return s


CASES = {"thresholds": case_thresholds, "covisibility": case_covisibility,
         "stale_scores": case_stale_scores, "collisions": case_collisions,
         "erase_reuse": case_erase_reuse, "rounding": case_rounding,
         "all_below": case_all_below}
CASE_SCORING = {"rounding": 5}  # every other case: L1, the scoring of ORBvoc.txt
VARIANTS = range(6)


def built_scripts():
    """-> [(name, scoring, script)]"""
    return [("%s-%d" % (name, v), CASE_SCORING.get(name, 0), fn(v))
            for name, fn in CASES.items() for v in VARIANTS]


def mixed_magnitude_pair(n=300, seed=0):
    """Two BowVectors over the same n words whose terms span many orders of magnitude, so that
    the double sum depends on the order of the adds."""
    rng = np.random.Generator(np.random.PCG64(900 + seed))
    ids = np.sort(rng.choice(5000, n, replace=False)).astype(np.int32)
    v1 = rng.uniform(0.1, 1.0, n) * 10.0 ** rng.integers(-9, 9, n)
    v2 = rng.uniform(0.1, 1.0, n) * 10.0 ** rng.integers(-9, 9, n)
    return ids, v1, ids.copy(), v2


def order_sensitive_pair(scoring):
    """A mixed-magnitude pair (L2: normalised) whose score has different double bits when the
    terms are summed in reverse and when they are summed pairwise."""
    for seed in range(50):
        i1, v1, i2, v2 = mixed_magnitude_pair(seed=seed)
        if scoring == 1:
            v1, v2 = v1 / np.sqrt((v1 * v1).sum()), v2 / np.sqrt((v2 * v2).sum())
        f = score(scoring, i1, v1, i2, v2, fused=False)
        if (f != score(scoring, i1, v1, i2, v2, fused=False, order="reverse")
                and f != score(scoring, i1, v1, i2, v2, fused=False, order="pairwise")):
            return i1, v1, i2, v2
    raise AssertionError("no pair found")


def contraction_pair(scoring, seed=0):
    """An L2 (normalised values) or dot-product pair on which fma(vi, wi, score) and the
    uncontracted product and sum give different doubles."""
    for s in range(seed, seed + 100):
        rng = np.random.Generator(np.random.PCG64(1300 + s))
        n = 40
        ids = np.sort(rng.choice(5000, n, replace=False)).astype(np.int32)
        v1, v2 = rng.uniform(0.05, 1.0, n), rng.uniform(0.05, 1.0, n)
        if scoring == 1:
            v1, v2 = v1 / np.sqrt((v1 * v1).sum()) * 0.9, v2 / np.sqrt((v2 * v2).sum()) * 0.9
        if score(scoring, ids, v1, ids, v2, True) != score(scoring, ids, v1, ids, v2, False):
            return ids, v1, ids.copy(), v2
    raise AssertionError("no pair found")


def random_bow(rng, nwords, n, lo=0):
    ids = np.sort(rng.choice(np.arange(lo, nwords), n, replace=False)).astype(np.int32)
    vals = rng.uniform(0.01, 1.0, n)
    return ids, vals / np.abs(vals).sum()


def seeded_script(seed, n_ops, nwords=600, nw=40, nkf0=0):
    """A seeded sequence of adds, erases, covisibility lists and queries over a small word range
    (so that keyframes share words), with ids that sometimes repeat (H19)."""
    rng = np.random.Generator(np.random.PCG64(7000 + seed))
    s, live, k = [], [], 0
    for _ in range(nkf0):
        s.append(("add", "k%d" % k, *random_bow(rng, nwords, nw)))
        live.append("k%d" % k)
        k += 1
    for name in live[::2]:  # half of the initial keyframes have neighbours
        s.append(("covis", name, [live[int(rng.integers(len(live)))]
                                  for _ in range(int(rng.integers(1, 11)))]))
    for _ in range(n_ops):
        r = rng.uniform()
        if r < 0.35 or len(live) < 3:
            s.append(("add", "k%d" % k, *random_bow(rng, nwords, int(rng.integers(1, nw + 1)))))
            live.append("k%d" % k)
            k += 1
        elif r < 0.45:
            s.append(("erase", live.pop(int(rng.integers(len(live))))))
        elif r < 0.65:
            n = int(rng.integers(0, 11))
            names = [None if rng.uniform() < 0.15 else live[int(rng.integers(len(live)))]
                     for _ in range(n)]
            s.append(("covis", live[int(rng.integers(len(live)))], names))
        elif r < 0.82:
            s.append(("reloc", int(rng.integers(0, 6)), *random_bow(rng, nwords, nw)))
        else:
            conn = [live[int(rng.integers(len(live)))] for _ in range(int(rng.integers(0, 4)))]
            s.append(("loop", int(rng.integers(0, 6)), *random_bow(rng, nwords, nw), conn,
                      float(rng.uniform(0.0, 0.05))))
    return s


# ==== the script file of tests/cpp/kfdb_test.cpp ================================================

def dump_script(path, scoring, script, ids=None):
    """Keyframe names become int64 ids (`ids`, default: the number in the name "k<number>");
    None (a neighbour that is not in the database) becomes an id nothing has."""
    ident = (lambda n: 10 ** 9 if n is None else int(n[1:])) if ids is None else \
        (lambda n: 10 ** 9 if n is None else ids[n])
    ops = [op for op in script if op[0] in ("add", "erase", "covis", "reloc", "loop")]
    with open(path, "wb") as f:
        np.array([scoring, len(ops)], np.int32).tofile(f)
        for op in ops:
            kind = ("add", "erase", "covis", "reloc", "loop").index(op[0])
            np.array([kind], np.int32).tofile(f)
            np.array([op[1] if kind >= 3 else ident(op[1])], np.int64).tofile(f)
            if kind in (0, 3, 4):
                np.array([len(op[2])], np.int32).tofile(f)
                np.asarray(op[2], np.int32).tofile(f)
                np.asarray(op[3], np.float64).tofile(f)
            if kind in (2, 4):
                lst = op[2] if kind == 2 else op[4]
                np.array([len(lst)], np.int32).tofile(f)
                np.array([ident(n) for n in lst], np.int64).tofile(f)
            if kind == 4:
                np.array([op[5]], np.float32).tofile(f)
