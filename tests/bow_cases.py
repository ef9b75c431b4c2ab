"""TemplatedVocabulary<FORB>::transform restated in plain numpy / Python from the reference's lines
(Thirdparty/DBoW2: TemplatedVocabulary.h:1140-1207 the loop over features, :1231-1272 the descent
of one feature; BowVector.cpp:34-46 addWeight, :50-58 addIfNotExist, :62-84 normalize;
FeatureVector.cpp:31-45 addFeature; ScoringObject.h:74-89 which scoring normalises how), with
branch counters and single-decision mutants; builders of synthetic vocabularies as node arrays
(complete and ragged trees, up to the ORBvoc shape k = 10, L = 6) and of the ORBvoc text format;
and the built cases that tests/test_bow_edges.py proves non-trivial on the CPU and runs against
bow_descend_kernel / bow_assemble_kernel on the GPU.

Node arrays are (parent, is_word, desc, weight) in insertion order: node 0 is the root,
parent[i] < i, a node's children are its nodes in ascending id (the order loadFromTextFile
pushes them, :1405), word ids are handed out to the flagged nodes in id order (:1421-1428) and
every other node keeps Node()'s word_id 0 (:329).

One choice is pinned here that the reference leaves open: transform(features, ..)
declares `NodeId nid;` without a value (:1164, :1192) and the descent writes it only when
nid_level <= 0 (:1240) or when it reaches nid_level (:1264), so a feature whose leaf lies above
nid_level gets an uninitialised node id.  The oracle and the kernel use 0; the mutant `nid_stale`
is the other plausible reading (the stack slot keeps the previous feature's value).
"""
from __future__ import annotations

import math

import numpy as np

SCORINGS = (0, 1, 2, 3, 4, 5)   # L1, L2, chi-square, KL, Bhattacharyya, dot product
WEIGHTINGS = (0, 1, 2, 3)       # TF_IDF, TF, IDF, BINARY
BOW_MAX = 4096                  # features per frame the library's assembly takes

MUTANTS = ("descent_le", "nid_high", "nid_low", "nid_stale", "w_ge", "tf_if_not_exist",
           "idf_add_weight", "count_times_w", "norm_descending", "l2_for_l1", "l1_for_l2",
           "nd_when_normalising", "stopped_in_fv", "nonword_dropped")

BRANCHES = ("tie", "shallow_leaf", "nid_root", "stopped", "repeated_word", "word0_nonword",
            "norm_zero")

_POP = np.array([bin(i).count("1") for i in range(256)], np.uint16)


def _bump(stats, key, by=1):
    if stats is not None and by:
        stats[key] = stats.get(key, 0) + int(by)


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def sparse_bits(rng, shape, planes=3):
    """Random bytes whose bits are set with probability 2**-planes: the AND of `planes` uniform
    byte planes (no per-bit random doubles)."""
    out = rng.integers(0, 256, shape, dtype=np.uint8)
    for _ in range(planes - 1):
        out &= rng.integers(0, 256, shape, dtype=np.uint8)
    return out


def vocab_arrays(k=10, L=6, seed=0, *, min_children=None, leaf_prob=0.0, nonword_prob=0.0,
                 inner_word_prob=0.0, dup_prob=0.0, stop_prob=0.03, interleave=False, planes=3):
    """(parent, is_word, desc, weight) of a k-ary tree of depth L, level by level.

    A child's descriptor is its parent's XOR the AND of `planes` random byte planes (about 12 % of
    the bits flip at planes = 3); level 1 is uniform.  The defaults give a complete tree whose
    level-L nodes are the words, 3 % of them stopped (weight 0).  Ragged trees:
      min_children     every inner node gets min_children..k children instead of k
      leaf_prob        a node above level L is childless with this probability
      nonword_prob     a childless node is not flagged a word, and keeps a positive weight
      inner_word_prob  a node with children is flagged a word (and takes a word id)
      dup_prob         a child repeats the descriptor of its elder sibling
      interleave       the nodes of a level are inserted in random order, so siblings' ids are
                       not contiguous
    """
    rng = _rng(seed)
    parent = [np.zeros(1, np.int32)]
    is_word = [np.zeros(1, np.uint8)]
    desc = [np.zeros((1, 32), np.uint8)]
    weight = [np.zeros(1, np.float64)]
    inner = np.zeros(1, np.int64)          # ids of the previous level's nodes that get children
    inner_desc = np.zeros((1, 32), np.uint8)
    nid = 1
    for level in range(1, L + 1):
        if len(inner) == 0:
            break
        if min_children is None:
            nch = np.full(len(inner), k, np.int64)
        else:
            nch = rng.integers(min_children, k + 1, len(inner))
        cnt = int(nch.sum())
        src = np.repeat(np.arange(len(inner)), nch)
        par = inner[src]
        if level == 1:
            d = rng.integers(0, 256, (cnt, 32), dtype=np.uint8)
        else:
            d = inner_desc[src] ^ sparse_bits(rng, (cnt, 32), planes)
        if dup_prob > 0:
            dup = (rng.uniform(size=cnt) < dup_prob) & (np.arange(cnt) > 0)
            dup[1:] &= src[1:] == src[:-1]
            for i in np.flatnonzero(dup):  # in order: a run of duplicates repeats its first
                d[i] = d[i - 1]
        if interleave:
            perm = rng.permutation(cnt)
            par, d = par[perm], d[perm]
        childless = np.ones(cnt, bool) if level == L else rng.uniform(size=cnt) < leaf_prob
        word = np.where(childless, rng.uniform(size=cnt) >= nonword_prob,
                        rng.uniform(size=cnt) < inner_word_prob)
        w = rng.uniform(0.5, 8.0, cnt)
        w[childless & word & (rng.uniform(size=cnt) < stop_prob)] = 0.0
        w[~childless & ~word] = 0.0
        parent.append(par.astype(np.int32))
        is_word.append(word.astype(np.uint8))
        desc.append(d)
        weight.append(w)
        ids = np.arange(nid, nid + cnt)
        inner, inner_desc = ids[~childless], d[~childless]
        nid += cnt
    return (np.concatenate(parent), np.concatenate(is_word),
            np.ascontiguousarray(np.concatenate(desc)), np.concatenate(weight))


def write_text(path, k, L, scoring, weighting, arrays, *, crlf=False, final_newline=True,
               blank_every=0, exp_weights=False):
    """The ORBvoc text format (saveToTextFile, :1442-1462): header "k L scoring weighting", one
    line per node "parent isLeaf d0 .. d31 weight".  Small trees only.  Weights are written so
    that strtod gives the same double back: repr, or 17 significant digits in exponent form."""
    parent, is_word, desc, weight = arrays
    assert len(parent) <= 12500, "write_text is for small trees"
    eol = "\r\n" if crlf else "\n"
    lines = [f"{k} {L} {scoring} {weighting}"]
    for i in range(1, len(parent)):
        w = float(weight[i])
        ws = "%.16e" % w if exp_weights else repr(w)
        assert float(ws) == w
        lines.append(f"{int(parent[i])} {int(is_word[i])} " + " ".join(map(str, desc[i].tolist()))
                     + " " + ws)
        if blank_every and i % blank_every == 0:
            lines.append("   " if i % (2 * blank_every) == 0 else "")
    text = eol.join(lines) + (eol if final_newline else "")
    with open(path, "w", newline="") as fh:
        fh.write(text)
    return path


class Tree:
    """Node arrays with the children of every node as a CSR in insertion order, and word ids."""

    def __init__(self, arrays):
        parent, is_word, desc, weight = arrays
        self.parent = np.asarray(parent, np.int64)
        n = len(self.parent)
        assert n >= 1 and (self.parent[1:] < np.arange(1, n)).all() and (self.parent[1:] >= 0).all()
        self.desc = np.ascontiguousarray(desc, np.uint8).reshape(n, 32)
        self.weight = np.asarray(weight, np.float64)
        flag = np.asarray(is_word, np.uint8).astype(bool).copy()
        flag[0] = False
        self.is_word = flag
        self.word = np.where(flag, np.cumsum(flag) - 1, 0).astype(np.int64)  # Node(): word_id 0
        self.nwords = int(flag.sum())
        self.child_ids = np.argsort(self.parent[1:], kind="stable") + 1     # ascending id per parent
        cnt = np.bincount(self.parent[1:], minlength=n) if n > 1 else np.zeros(n, np.int64)
        self.child_off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
        self.nodes = n


def as_tree(arrays) -> Tree:
    return arrays if isinstance(arrays, Tree) else Tree(arrays)


def hamming(a, b):
    """FORB::distance (FORB.cpp:81-101) row by row."""
    return _POP[a ^ b].sum(axis=-1, dtype=np.int64)


def descend(tree, desc, last_min=False, stats=None):
    """The descent of :1245-1267 for every descriptor at once, one level at a time: at each level
    the children in insertion order, strict '<' so the first closest child wins (last_min: the
    `<=` mutant).  -> (leaf node, its level, path) with path[i, l - 1] the node of feature i at
    level l, or -1 below its leaf."""
    t = as_tree(tree)
    d = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
    n = len(d)
    node = np.zeros(n, np.int64)
    leaf_level = np.zeros(n, np.int64)
    active = np.arange(n)
    cols = []
    level = 0
    while len(active):
        level += 1
        cur = node[active]
        c0 = t.child_off[cur]
        cnt = t.child_off[cur + 1] - c0
        assert (cnt > 0).all()
        width = int(cnt.max())
        dist = np.full((len(active), width), 1 << 30, np.int64)
        for j in range(width):
            ok = j < cnt
            ch = t.child_ids[c0[ok] + j]
            dist[ok, j] = hamming(d[active[ok]], t.desc[ch])
        best = dist.min(axis=1)
        if last_min:
            pick = width - 1 - np.argmin(dist[:, ::-1], axis=1)
        else:
            pick = np.argmin(dist, axis=1)       # the first minimum
        ties = (dist == best[:, None]).sum(axis=1) > 1
        _bump(stats, "tie", ties.sum())
        _bump(stats, "tie_level_%d" % level, ties.sum())
        node[active] = t.child_ids[c0 + pick]
        col = np.full(n, -1, np.int64)
        col[active] = node[active]
        cols.append(col)
        leaf_level[active] = level
        more = t.child_off[node[active] + 1] > t.child_off[node[active]]
        active = active[more]
    path = np.stack(cols, axis=1) if cols else np.zeros((n, 0), np.int64)
    return node, leaf_level, path


def transform(arrays, L, scoring, weighting, desc, levelsup, mutant=None, stats=None):
    """transform(features, BowVector, FeatureVector, levelsup) -> the five arrays of
    Vocabulary.transform: (word_ids, values, node_ids, node_off, feat).  Every double sum is made
    of Python additions in the reference's order, so the values compare bit for bit."""
    assert mutant is None or mutant in MUTANTS
    t = as_tree(arrays)
    d = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
    n = len(d)
    bow, fv = {}, {}
    if t.nwords > 0:                                         # empty() (:1147)
        must = scoring != 5                                  # DotProductScoring (ScoringObject.h:89)
        l2 = scoring == 1                                    # L2Scoring (:77); L1 for the others
        if mutant == "l2_for_l1" and scoring != 1:
            l2 = True
        if mutant == "l1_for_l2" and scoring == 1:
            l2 = False
        tf = weighting in (0, 1)                             # :1158
        add_weight = tf
        if mutant == "tf_if_not_exist" and tf:
            add_weight = False
        if mutant == "idf_add_weight" and not tf:
            add_weight = True
        leaf, leaf_level, path = descend(t, d, last_min=mutant == "descent_le", stats=stats)
        nid_level = L - levelsup                             # :1239
        store = nid_level - 1 if mutant == "nid_high" else nid_level + 1 if mutant == "nid_low" else nid_level
        count = {}
        prev_nid = 0
        for i in range(n):
            if nid_level <= 0:                               # :1240
                nid = 0
                _bump(stats, "nid_root")
            elif 1 <= store <= leaf_level[i]:                # :1264
                nid = int(path[i, store - 1])
            elif store > leaf_level[i]:                      # never written (H20): 0
                _bump(stats, "shallow_leaf")
                nid = prev_nid if mutant == "nid_stale" else 0
            else:
                nid = 0
            prev_nid = nid
            node = int(leaf[i])
            w = float(t.weight[node])                        # :1271
            word = int(t.word[node])                         # :1270
            nonword = not t.is_word[node]
            keep = w >= 0 if mutant == "w_ge" else w > 0     # :1170
            if not keep:
                _bump(stats, "stopped")
                if mutant == "stopped_in_fv":
                    fv.setdefault(nid, []).append(i)
                continue
            if nonword:
                _bump(stats, "word0_nonword")
                if mutant == "nonword_dropped":
                    continue
            if word in bow:
                _bump(stats, "repeated_word")
                count[word] += 1
                if add_weight:
                    bow[word] = bow[word] + w                # addWeight (BowVector.cpp:40)
            else:
                bow[word] = w                                # :44 / :56
                count[word] = 1
            fv.setdefault(nid, []).append(i)                 # addFeature (FeatureVector.cpp:31-45)
        keys = sorted(bow)
        if mutant == "count_times_w" and add_weight:
            first = {}
            for i in range(n):  # the first kept feature of each word
                node = int(leaf[i])
                if float(t.weight[node]) > 0:
                    first.setdefault(int(t.word[node]), float(t.weight[node]))
            bow = {kk: count[kk] * first[kk] for kk in keys}
        if tf and bow and (not must or mutant == "nd_when_normalising"):
            nd = float(len(bow))                             # :1177-1183
            bow = {kk: bow[kk] / nd for kk in keys}
        if must:                                             # normalize (BowVector.cpp:62-84)
            norm = 0.0
            order = keys[::-1] if mutant == "norm_descending" else keys
            if l2:
                for kk in order:
                    norm += bow[kk] * bow[kk]
                norm = math.sqrt(norm)
            else:
                for kk in order:
                    norm += abs(bow[kk])
            if norm > 0.0:
                bow = {kk: bow[kk] / norm for kk in keys}
            else:
                _bump(stats, "norm_zero")
    return as_arrays(bow, fv)


def as_arrays(bow, fv):
    wk, nk = sorted(bow), sorted(fv)
    wid = np.array(wk, np.int32)
    val = np.array([bow[k] for k in wk], np.float64)
    nid = np.array(nk, np.int32)
    off = np.concatenate([[0], np.cumsum([len(fv[k]) for k in nk])]).astype(np.int32)
    feat = np.array([i for k in nk for i in fv[k]], np.int32)
    return wid, val, nid, off, feat


def same(a, b):
    """Two transform results equal, doubles by their bits."""
    if len(a) != len(b):
        return False
    for x, y in zip(a, b):
        x, y = np.asarray(x), np.asarray(y)
        if x.shape != y.shape:
            return False
        if y.dtype == np.float64:
            if not np.array_equal(np.asarray(x, np.float64).view(np.uint64), y.view(np.uint64)):
                return False
        elif not np.array_equal(x, y):
            return False
    return True


def noisy(rng, desc, planes=4):
    """Copies of descriptors with each bit flipped with probability 2**-planes."""
    d = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
    return d ^ sparse_bits(rng, d.shape, planes)


def clustered_queries(tree, rng, n, clusters, planes=4):
    """n descriptors in clusters: noisy copies of `clusters` random childless nodes, so several
    features share a word."""
    t = as_tree(tree)
    childless = np.flatnonzero(t.child_off[1:] == t.child_off[:-1])
    centre = rng.choice(childless, clusters, replace=False)
    return noisy(rng, t.desc[centre[rng.integers(0, clusters, n)]], planes)


# ---------------------------------------------------------------------------------------------
# the built cases: name -> dict(k, L, scoring, weighting, arrays, desc, levelsups)

def _case(k, L, scoring, weighting, arrays, desc, levelsups):
    return dict(k=k, L=L, scoring=scoring, weighting=weighting, arrays=arrays,
                desc=np.ascontiguousarray(desc, np.uint8).reshape(-1, 32), levelsups=tuple(levelsups))


def levelsups_of(L):
    return (0, 1, L - 1, L, L + 1, 100)


def complete_tree():
    return vocab_arrays(6, 4, seed=11)


def ragged_tree():
    """1..5 children, leaves at every depth, childless nodes that are no words, word-flagged nodes
    with children, duplicated siblings, interleaved insertion."""
    return vocab_arrays(5, 4, seed=22, min_children=1, leaf_prob=0.3, nonword_prob=0.25,
                        inner_word_prob=0.3, dup_prob=0.15, stop_prob=0.1, interleave=True)


def bit_tree(k=3, L=4):
    """Child j of a node at level l is the node's descriptor with bit k (l - 1) + j flipped: the
    all-zero, the all-one and every inner node's descriptor are equidistant from all children
    of the nodes on their way down."""
    parent, desc = [0], [np.zeros(32, np.uint8)]
    prev = [0]
    for level in range(1, L + 1):
        cur = []
        for p in prev:
            for j in range(k):
                b = k * (level - 1) + j
                d = desc[p].copy()
                d[b >> 3] ^= np.uint8(1 << (b & 7))
                cur.append(len(parent))
                parent.append(p)
                desc.append(d)
        prev = cur
    n = len(parent)
    is_word = np.zeros(n, np.uint8)
    is_word[prev] = 1
    weight = np.zeros(n)
    weight[prev] = 0.25 + np.arange(len(prev)) * 0.37
    return np.array(parent, np.int32), is_word, np.stack(desc), weight


def ties_case():
    """Duplicated siblings, queries equal to centroids, all-zero and all-one descriptors."""
    arrays = vocab_arrays(5, 4, seed=13, dup_prob=0.5, stop_prob=0.05)
    arrays[2][2] = arrays[2][1]                              # level 1: nodes 1 and 2 are twins
    t = Tree(arrays)
    rng = _rng(131)
    pick = rng.choice(np.arange(1, t.nodes), 120, replace=False)
    desc = np.concatenate([t.desc[1:3], t.desc[pick], noisy(rng, t.desc[pick[:60]]),
                           np.zeros((2, 32), np.uint8), np.full((2, 32), 255, np.uint8)])
    return _case(5, 4, 0, 0, arrays, desc, (2, 0, 4))


def ties_bits_case():
    arrays = bit_tree(3, 4)
    t = Tree(arrays)
    inner = np.flatnonzero(t.child_off[1:] > t.child_off[:-1])
    desc = np.concatenate([np.zeros((1, 32), np.uint8), np.full((1, 32), 255, np.uint8),
                           t.desc[inner], t.desc[inner] ^ np.uint8(0x80)])
    return _case(3, 4, 1, 1, arrays, desc, (1, 2, 3))


def nonword_case(weighting=0, scoring=0):
    """The ragged tree queried with exact and noisy copies of its childless nodes, the real word 0
    and the childless non-word nodes in turn, so that word 0's value is a sum of different
    weights in feature order."""
    arrays = ragged_tree()
    t = Tree(arrays)
    rng = _rng(121)
    childless = np.flatnonzero(t.child_off[1:] == t.child_off[:-1])
    leaf, _, _ = descend(t, t.desc[childless])
    home = childless[leaf == childless]                      # copies that reach their own node
    nonword = home[~t.is_word[home] & (t.weight[home] > 0)]
    word0 = home[t.is_word[home] & (t.word[home] == 0) & (t.weight[home] > 0)]
    assert len(nonword) >= 3 and len(word0) == 1
    turn = np.array([word0[0], nonword[0], word0[0], nonword[1], nonword[0], word0[0], nonword[2]])
    desc = np.concatenate([t.desc[turn], noisy(rng, t.desc[childless]), t.desc[turn[::-1]],
                           clustered_queries(t, rng, 150, 25)])
    return _case(5, 4, scoring, weighting, arrays, desc, levelsups_of(4))


def stop_cases():
    arrays = vocab_arrays(5, 3, seed=14, stop_prob=0.5)
    t = Tree(arrays)
    rng = _rng(141)
    q = clustered_queries(t, rng, 400, 60)
    leaf, _, _ = descend(t, q)
    kept = t.weight[leaf] > 0
    a, b = q[kept], q[~kept]
    m = min(len(a), len(b), 90)
    inter = np.empty((2 * m, 32), np.uint8)
    inter[0::2], inter[1::2] = b[:m], a[:m]
    single = np.concatenate([b[:40], a[:1], b[40:75]])
    allzero = (arrays[0], arrays[1], arrays[2], np.zeros_like(arrays[3]))
    return {
        "stop_all": _case(5, 3, 0, 0, allzero, q[:130], (1, 0)),
        "stop_half": _case(5, 3, 0, 0, arrays, inter, (1, 3)),
        "stop_single_kept": _case(5, 3, 1, 1, arrays, single, (2,)),
    }


def empty_cases():
    root = (np.zeros(1, np.int32), np.zeros(1, np.uint8), np.zeros((1, 32), np.uint8), np.zeros(1))
    arrays = vocab_arrays(4, 2, seed=15)
    noflag = (arrays[0], np.zeros_like(arrays[1]), arrays[2], np.full(len(arrays[0]), 1.5))
    q = _rng(151).integers(0, 256, (70, 32), dtype=np.uint8)
    return {
        "empty_root": _case(4, 2, 0, 0, root, q, (0, 1)),
        "empty_noflag": _case(4, 2, 0, 0, noflag, q, (0, 1)),
    }


def heavy_tree():
    """A k = 4, L = 2 tree whose words all weigh 0.1: 0.1 added 6 times is not 6 * 0.1."""
    p, f, d, w = vocab_arrays(4, 2, seed=16, stop_prob=0.0)
    return p, f, d, np.where(f > 0, 0.1, 0.0)


def heavy_queries(n=BOW_MAX, split=(1500, 1500, 1096), seed=161):
    """-> (n copies of one descriptor, n descriptors over three words in runs of `split`,
    shuffled in feature order)."""
    t = Tree(heavy_tree())
    leaves = np.flatnonzero(t.is_word)
    leaf, _, _ = descend(t, t.desc[leaves])
    home = leaves[leaf == leaves][[0, 5, 11]]
    assert len(set(t.word[home])) == 3 and sum(split) == n
    three = np.repeat(t.desc[home], split, axis=0)
    return np.repeat(t.desc[home[1:2]], n, axis=0), three[_rng(seed).permutation(n)]


def extreme_tree():
    """One level, six words: 5e-324, 1e-310, 1e300, 3.0, 1e-310, 5e-324."""
    d = _rng(17).integers(0, 256, (7, 32), dtype=np.uint8)
    w = np.array([0.0, 5e-324, 1e-310, 1e300, 3.0, 1e-310, 5e-324])
    return np.zeros(7, np.int32), np.array([0, 1, 1, 1, 1, 1, 1], np.uint8), d, w


def extreme_cases():
    arrays = extreme_tree()
    d = arrays[2]
    mixed = d[[1, 2, 3, 4, 1, 1, 2, 5, 6, 3, 1]]          # 1e300 twice: its square is inf
    tiny = d[[1, 2, 1, 6, 5, 1, 2, 2, 6]]                 # denormals only: the squares are 0
    out = {}
    for sc, tag in ((0, "l1"), (1, "l2")):
        for wt, wtag in ((0, "tfidf"), (2, "idf")):
            out[f"extreme_mixed_{tag}_{wtag}"] = _case(6, 1, sc, wt, arrays, mixed, (0, 1))
            out[f"extreme_tiny_{tag}_{wtag}"] = _case(6, 1, sc, wt, arrays, tiny, (0,))
    return out


def grid_queries():
    t = Tree(complete_tree())
    return clustered_queries(t, _rng(111), 260, 70)


def built_cases():
    """The small cases over which the mutant and coverage tests run (and which the oracle can
    load as text)."""
    cases = {}
    comp, q = complete_tree(), grid_queries()
    for sc in SCORINGS:
        for wt in WEIGHTINGS:
            cases[f"grid_s{sc}_w{wt}"] = _case(6, 4, sc, wt, comp, q, (2,))
    cases["levelsup_complete"] = _case(6, 4, 0, 0, comp, q[:120], levelsups_of(4))
    cases["levelsup_ragged"] = nonword_case()
    cases["nonword_tf_l2"] = nonword_case(weighting=1, scoring=1)
    cases["nonword_idf_dot"] = nonword_case(weighting=2, scoring=5)
    cases["ties"] = ties_case()
    cases["ties_bits"] = ties_bits_case()
    cases.update(stop_cases())
    cases.update(empty_cases())
    cases.update(extreme_cases())
    one, _ = heavy_queries()
    for wt in (1, 2, 3):
        cases[f"heavy_small_w{wt}"] = _case(4, 2, 5, wt, heavy_tree(),
                                            np.concatenate([one[:6], grid_queries()[:40]]), (1,))
    return cases


def production_case(seed=3, n=1000, clusters=280):
    """k = 10, L = 6: 10**6 words (ORBvoc's shape), queried with noisy copies of random words."""
    arrays = vocab_arrays(10, 6, seed=seed)
    t = Tree(arrays)
    desc = clustered_queries(t, _rng(seed + 1000), n, clusters)
    return t, desc
