"""The BoW transform (bow_descend_kernel, bow_assemble_kernel, orbfe_bow.hip) pinned at its edges:
the ORBvoc shape (k = 10, L = 6, 10^6 words), ragged trees, descent ties, nodes that are no words,
stop words, empty vocabularies, thousands of features on one word, extreme weights, the size seams
of the LDS sort and scan, and the two loaders against the arrays constructor.

The reference of every GPU comparison is tests/bow_cases.py's restatement of
TemplatedVocabulary.h:1140-1207, :1231-1272, bit for bit; trees small enough to write as text are
checked against the C oracle too.  The CPU tests prove the restatement equal to the oracle, every
single-decision mutant visible and every branch reached on the built cases.
"""
import numpy as np
import pytest

import bow_cases as B
import kfdb_cases as K
import oracle

CASES = B.built_cases()
TEXT_MAX = 12500  # nodes up to which a tree is also written as text for the oracle


def check_same(got, want, what=""):
    assert B.same(got, want), (what, [np.asarray(x).tolist()[:8] for x in got],
                               [np.asarray(x).tolist()[:8] for x in want])


def oracle_vocab(case, tmp_path, **opts):
    path = str(tmp_path / "voc.txt")
    B.write_text(path, case["k"], case["L"], case["scoring"], case["weighting"], case["arrays"], **opts)
    return oracle.Vocabulary(path), path


def expected(case, levelsup, tmp_path, stats=None, desc=None):
    """The restatement's transform; for text-sized trees asserted equal to the oracle's."""
    d = case["desc"] if desc is None else desc
    want = B.transform(case["arrays"], case["L"], case["scoring"], case["weighting"], d, levelsup,
                       stats=stats)
    if len(case["arrays"][0]) <= TEXT_MAX:
        ov, _ = oracle_vocab(case, tmp_path)
        check_same(ov.transform(d, levelsup), want, "oracle vs restatement")
    return want


# ---------------------------------------------------------------------------------------------
# CPU

@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_vs_oracle(name, tmp_path):
    case = CASES[name]
    t = B.Tree(case["arrays"])
    ov, _ = oracle_vocab(case, tmp_path)
    assert (ov.k, ov.L, ov.nodes, ov.words) == (case["k"], case["L"], t.nodes, t.nwords)
    for levelsup in case["levelsups"]:
        want = B.transform(t, case["L"], case["scoring"], case["weighting"], case["desc"], levelsup)
        check_same(ov.transform(case["desc"], levelsup), want, (name, levelsup))


def test_restatement_vs_oracle_heavy(tmp_path):
    """4096 features on one word and on three (1500 / 1500 / 1096), every weighting."""
    one, three = B.heavy_queries()
    for wt in B.WEIGHTINGS:
        for sc in (0, 5):
            case = B._case(4, 2, sc, wt, B.heavy_tree(), one, (1,))
            ov, _ = oracle_vocab(case, tmp_path)
            for d in (one, three):
                want = B.transform(case["arrays"], 2, sc, wt, d, 1)
                check_same(ov.transform(d, 1), want, (wt, sc))
                assert len(want[0]) == (1 if d is one else 3) and len(want[4]) == B.BOW_MAX


def _all_outputs(mutant=None):
    out = []
    for name in sorted(CASES):
        c = CASES[name]
        t = B.Tree(c["arrays"])
        for levelsup in c["levelsups"]:
            out.append((name, levelsup, B.transform(t, c["L"], c["scoring"], c["weighting"],
                                                    c["desc"], levelsup, mutant=mutant)))
    return out


@pytest.fixture(scope="module")
def baseline_outputs():
    return _all_outputs()


@pytest.mark.parametrize("mutant", B.MUTANTS)
def test_mutant_changes_some_output(mutant, baseline_outputs):
    changed = [(n, l) for (n, l, a), (_, _, b) in zip(baseline_outputs, _all_outputs(mutant))
               if not B.same(a, b)]
    assert changed, mutant


def test_every_branch_is_reached():
    stats = {}
    for name in sorted(CASES):
        c = CASES[name]
        for levelsup in c["levelsups"]:
            B.transform(c["arrays"], c["L"], c["scoring"], c["weighting"], c["desc"], levelsup,
                        stats=stats)
    for br in B.BRANCHES:
        assert stats.get(br, 0) > 0, (br, stats)


def test_built_cases_hold_what_they_claim():
    def stats_of(name, levelsup):
        c, st = CASES[name], {}
        out = B.transform(c["arrays"], c["L"], c["scoring"], c["weighting"], c["desc"], levelsup, stats=st)
        return c, st, out
    for name in ("ties", "ties_bits"):
        c, st, _ = stats_of(name, CASES[name]["levelsups"][0])
        for level in range(1, c["L"] + 1):
            assert st.get("tie_level_%d" % level, 0) > 0, (name, level, st)
    c, st, out = stats_of("levelsup_ragged", 0)          # nid_level = L: the shallow leaves
    assert st["shallow_leaf"] >= 5 and st["word0_nonword"] >= 10 and st["repeated_word"] >= 10
    t = B.Tree(c["arrays"])
    assert (t.is_word & (t.child_off[1:] > t.child_off[:-1])).any()   # a word-flagged inner node
    assert out[0][0] == 0                                  # word 0 holds the merged value
    c, st, out = stats_of("stop_all", 1)
    assert st["stopped"] == len(c["desc"]) and st["norm_zero"] == 1
    assert [len(x) for x in out] == [0, 0, 0, 1, 0] and out[3][0] == 0
    c, st, out = stats_of("stop_half", 1)
    assert st["stopped"] == len(c["desc"]) // 2 >= 40
    c, st, out = stats_of("stop_single_kept", 2)
    assert st["stopped"] == len(c["desc"]) - 1 and len(out[0]) == 1 and out[4].tolist() == [40]
    for name in ("empty_root", "empty_noflag"):
        assert [len(x) for x in stats_of(name, 0)[2]] == [0, 0, 0, 1, 0]
    _, st, out = stats_of("extreme_mixed_l2_tfidf", 0)
    assert (out[1] == 0).all() and len(out[1]) == 6       # the norm is inf
    _, st, out = stats_of("extreme_tiny_l2_tfidf", 0)
    assert st["norm_zero"] == 1 and (out[1] > 0).all() and (out[1] < 1e-300).all()
    _, st, out = stats_of("extreme_tiny_l1_tfidf", 0)
    assert "norm_zero" not in st and abs(out[1].sum() - 1) < 1e-9


def check_production(t, desc):
    """What the depth-6 case must hold before it is worth a GPU call."""
    assert (t.nodes, t.nwords) == (1111111, 10 ** 6)
    leaf, level, _ = B.descend(t, desc)
    assert (level == 6).all()
    words = t.word[leaf]
    kept = t.weight[leaf] > 0
    assert (words > 1 << 16).any() and (words > 1 << 19).any()
    _, cnt = np.unique(words[kept], return_counts=True)
    assert (cnt > 1).sum() >= 100
    assert (~kept).sum() >= 10


@pytest.fixture(scope="module")
def production():
    t, desc = B.production_case()
    check_production(t, desc)
    return t, desc


def test_production_case_properties(production):
    t, desc = production
    for levelsup in (4, 0):
        wid, val, nid, off, feat = B.transform(t, 6, 0, 0, desc, levelsup)
        assert len(wid) > 300 and abs(val.sum() - 1) < 1e-9 and nid.max() > (11111 if levelsup == 0 else 11)


TEXT_OPTIONS = {
    "plain": {},
    "crlf": dict(crlf=True),
    "no_final_newline": dict(final_newline=False),
    "blank_lines": dict(blank_every=7),
    "exponent_weights": dict(exp_weights=True),
    "all": dict(crlf=True, final_newline=False, blank_every=5, exp_weights=True),
}


def _bad_parent_arrays():
    p, f, d, w = (x.copy() for x in B.vocab_arrays(3, 2, seed=18))
    p[5] = 5
    return p, f, d, w


REFUSED = {  # name: (header k, L, scoring, weighting, arrays)
    "parent_is_self": lambda: (3, 2, 0, 0, _bad_parent_arrays()),
    "k21": lambda: (21, 2, 0, 0, B.vocab_arrays(3, 2, seed=18)),
    "L11": lambda: (3, 11, 0, 0, B.vocab_arrays(3, 2, seed=18)),
    "scoring6": lambda: (3, 2, 6, 0, B.vocab_arrays(3, 2, seed=18)),
}


@pytest.mark.parametrize("opt", sorted(TEXT_OPTIONS))
def test_oracle_loader_text_options(opt, tmp_path):
    case = CASES["levelsup_ragged"]
    t = B.Tree(case["arrays"])
    ov, _ = oracle_vocab(case, tmp_path, **TEXT_OPTIONS[opt])
    assert (ov.k, ov.L, ov.scoring, ov.weighting, ov.nodes, ov.words) == (5, 4, 0, 0, t.nodes, t.nwords)
    check_same(ov.transform(case["desc"], 2), B.transform(t, 4, 0, 0, case["desc"], 2), opt)


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_oracle_loader_refuses(name, tmp_path):
    from orbslam_mapsave_amd.abi import ORBFE_ERR_ARG, OrbfeError
    k, L, sc, wt, arrays = REFUSED[name]()
    path = B.write_text(str(tmp_path / "bad.txt"), k, L, sc, wt, arrays)
    with pytest.raises(OrbfeError) as e:
        oracle.Vocabulary(path)
    assert e.value.status == ORBFE_ERR_ARG


# ---------------------------------------------------------------------------------------------
# GPU

def gpu_vocab(case):
    from orbslam_mapsave_amd.native import Vocabulary
    gv = Vocabulary.from_arrays(case["k"], case["L"], case["scoring"], case["weighting"],
                                *case["arrays"], device=0)
    t = B.Tree(case["arrays"])
    assert (gv.k, gv.L, gv.scoring, gv.weighting, gv.nodes, gv.words) == (
        case["k"], case["L"], case["scoring"], case["weighting"], t.nodes, t.nwords)
    return gv


def run_case(case, tmp_path):
    gv = gpu_vocab(case)
    try:
        for levelsup in case["levelsups"]:
            check_same(gv.transform(case["desc"], levelsup), expected(case, levelsup, tmp_path),
                       levelsup)
    finally:
        gv.close()


def batch_transform(gv, slots, cap, levelsup):
    """orbfe_bow_transform_batch_device over the descriptor sets `slots` -> one result per slot."""
    import torch
    dev = torch.device("cuda", 0)
    S_ = len(slots)
    d = np.zeros((S_, cap, 32), np.uint8)
    for i, x in enumerate(slots):
        d[i, :len(x)] = x
    D = torch.from_numpy(d).to(dev)
    N = torch.tensor([len(x) for x in slots], dtype=torch.int32, device=dev)
    wid = torch.full((S_, cap), -7, dtype=torch.int32, device=dev)
    val = torch.full((S_, cap), -7.0, dtype=torch.float64, device=dev)
    nid = torch.full((S_, cap), -7, dtype=torch.int32, device=dev)
    off = torch.full((S_, cap + 1), -7, dtype=torch.int32, device=dev)
    feat = torch.full((S_, cap), -7, dtype=torch.int32, device=dev)
    nw = torch.full((S_,), -7, dtype=torch.int32, device=dev)
    nn = torch.full((S_,), -7, dtype=torch.int32, device=dev)
    gv.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    try:
        gv.transform_batch_device(S_, D.data_ptr(), N.data_ptr(), cap, levelsup, wid.data_ptr(),
                                  val.data_ptr(), nw.data_ptr(), nid.data_ptr(), off.data_ptr(),
                                  feat.data_ptr(), nn.data_ptr())
        torch.cuda.synchronize()
    finally:
        gv.set_stream(None)
    out = []
    for i in range(S_):
        w, n_ = int(nw[i]), int(nn[i])
        assert 0 <= w <= len(slots[i]) and 0 <= n_ <= len(slots[i])
        o = off[i, :n_ + 1].cpu().numpy()
        out.append((wid[i, :w].cpu().numpy(), val[i, :w].cpu().numpy(), nid[i, :n_].cpu().numpy(),
                    o, feat[i, :o[-1]].cpu().numpy()))
    return out


@pytest.fixture(scope="module")
def production_gpu(production):
    """The depth-6 vocabulary, built and uploaded once; its properties are asserted first."""
    from orbslam_mapsave_amd.native import Vocabulary
    t, desc = production
    check_production(t, desc)
    gv = Vocabulary.from_arrays(10, 6, 0, 0, t.parent.astype(np.int32), t.is_word.astype(np.uint8),
                                t.desc, t.weight, device=0)
    assert (gv.k, gv.L, gv.nodes, gv.words) == (10, 6, t.nodes, t.nwords)
    yield gv, t, desc
    gv.close()


@pytest.mark.gpu
@pytest.mark.parametrize("zc", ["1", "0"])
@pytest.mark.parametrize("levelsup", [4, 0])
def test_gpu_production_transform(levelsup, zc, production_gpu, monkeypatch):
    monkeypatch.setenv("ORBFE_ZERO_COPY", zc)
    gv, t, desc = production_gpu
    want = B.transform(t, 6, 0, 0, desc, levelsup)
    assert want[0].max() > 1 << 19
    check_same(gv.transform(desc, levelsup), want)


@pytest.mark.gpu
def test_gpu_production_batch(production_gpu):
    gv, t, desc = production_gpu
    slots = [desc, desc[:333], desc[500:]]
    for levelsup in (4, 0):
        got = batch_transform(gv, slots, 1100, levelsup)
        for g, d in zip(got, slots):
            check_same(g, B.transform(t, 6, 0, 0, d, levelsup))


@pytest.mark.gpu
def test_gpu_production_score_and_database(production_gpu):
    """Two depth-6 BowVectors through Vocabulary.score and into a KeyFrameDatabase, whose add
    checks the word ids against the word count."""
    from orbslam_mapsave_amd.native import KeyFrameDatabase
    gv, t, desc = production_gpu
    a = gv.transform(desc[:700], 4)
    b = gv.transform(desc[300:], 4)
    check_same(a, B.transform(t, 6, 0, 0, desc[:700], 4))
    assert len(np.intersect1d(a[0], b[0])) > 50
    got = gv.score(a[0], a[1], b[0], b[1])
    want = K.score(0, a[0], a[1], b[0], b[1])
    assert 0 < want < 1 and np.float64(got).view(np.uint64) == np.float64(want).view(np.uint64)
    db = KeyFrameDatabase(gv, 1024)
    try:
        assert db.add(a[0], a[1]) == 0 and db.add(b[0], b[1]) == 1 and len(db) == 2
    finally:
        db.close()


@pytest.mark.gpu
@pytest.mark.parametrize("wt", B.WEIGHTINGS)
@pytest.mark.parametrize("sc", B.SCORINGS)
def test_gpu_scoring_weighting_grid(sc, wt, tmp_path):
    run_case(CASES[f"grid_s{sc}_w{wt}"], tmp_path)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["levelsup_complete", "levelsup_ragged"])
def test_gpu_levelsup(name, tmp_path):
    """levelsup 0, 1, L - 1, L, L + 1 and 100; the ragged tree has leaves above nid_level, whose
    node id is the pinned 0."""
    case = CASES[name]
    assert case["levelsups"] == (0, 1, 3, 4, 5, 100)
    run_case(case, tmp_path)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["ties", "ties_bits"])
def test_gpu_descent_ties(name, tmp_path):
    case = CASES[name]
    st = {}
    B.transform(case["arrays"], case["L"], case["scoring"], case["weighting"], case["desc"], 0, stats=st)
    assert all(st.get("tie_level_%d" % l, 0) > 0 for l in range(1, case["L"] + 1)), st
    run_case(case, tmp_path)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["levelsup_ragged", "nonword_tf_l2", "nonword_idf_dot"])
def test_gpu_nonword_and_word_flagged_nodes(name, tmp_path):
    """A childless node that is no word lands in word 0 with its own weight, merged with the real
    word 0 in feature order; a word-flagged node with children is descended through."""
    case = CASES[name]
    st = {}
    want = B.transform(case["arrays"], case["L"], case["scoring"], case["weighting"], case["desc"], 2, stats=st)
    assert st["word0_nonword"] >= 10 and want[0][0] == 0
    run_case(case, tmp_path)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["stop_all", "stop_half", "stop_single_kept"])
def test_gpu_stop_words(name, tmp_path):
    case = CASES[name]
    run_case(case, tmp_path)
    if name == "stop_all":
        gv = gpu_vocab(case)
        try:
            got = [gv.transform(case["desc"], 1)]
            got += batch_transform(gv, [case["desc"], case["desc"][:3]], 200, 1)
        finally:
            gv.close()
        for wid, val, nid, off, feat in got:
            assert len(wid) == len(val) == len(nid) == len(feat) == 0 and off.tolist() == [0]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["empty_root", "empty_noflag"])
def test_gpu_empty_vocabulary(name, tmp_path):
    case = CASES[name]
    gv = gpu_vocab(case)
    try:
        assert gv.words == 0
        for levelsup in case["levelsups"]:
            for d in (case["desc"], case["desc"][:0]):
                got = gv.transform(d, levelsup)
                assert [len(x) for x in got] == [0, 0, 0, 1, 0] and got[3][0] == 0
        for g in batch_transform(gv, [case["desc"], case["desc"][:1]], 80, 1):
            assert [len(x) for x in g] == [0, 0, 0, 1, 0] and g[3][0] == 0
    finally:
        gv.close()
    run_case(case, tmp_path)


@pytest.mark.gpu
@pytest.mark.parametrize("sc", [0, 5])
@pytest.mark.parametrize("wt", [1, 2, 3, 0])
def test_gpu_heavy_repetition(wt, sc, tmp_path):
    """4096 features on one word (w = 0.1 added 4096 times under TF) and on three words in runs of
    1500 / 1500 / 1096, which straddle the scan chunks at 1024 and 2048."""
    one, three = B.heavy_queries()
    case = B._case(4, 2, sc, wt, B.heavy_tree(), one, (1,))
    gv = gpu_vocab(case)
    try:
        for d in (one, three):
            check_same(gv.transform(d, 1), expected(case, 1, tmp_path, desc=d))
    finally:
        gv.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(n for n in CASES if n.startswith("extreme_")))
def test_gpu_extreme_weights(name, tmp_path):
    run_case(CASES[name], tmp_path)


SIZES = (0, 1, 2, 3, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096)


@pytest.fixture(scope="module")
def size_case(tmp_path_factory):
    """One text-sized vocabulary and 4097 clustered descriptors; the expected result per n, asserted
    equal between restatement and oracle."""
    arrays = B.complete_tree()
    pool = B.clustered_queries(B.Tree(arrays), B._rng(191), B.BOW_MAX + 1, 900)
    case = B._case(6, 4, 0, 0, arrays, pool, (2,))
    tmp = tmp_path_factory.mktemp("sizes")
    want = {n: expected(case, 2, tmp, desc=pool[:n]) for n in SIZES}
    return case, pool, want


@pytest.mark.gpu
@pytest.mark.parametrize("zc", ["1", "0"])
def test_gpu_sizes_one_handle(zc, size_case, monkeypatch):
    """Ascending, then descending, on one handle: the pinned block and the scratch buffers grow
    and are reused; the padding seams of the sort and the chunk seams of the scan."""
    from orbslam_mapsave_amd.abi import ORBFE_ERR_UNSUPPORTED
    from orbslam_mapsave_amd.native import OrbfeError
    monkeypatch.setenv("ORBFE_ZERO_COPY", zc)
    case, pool, want = size_case
    gv = gpu_vocab(case)
    try:
        for n in SIZES + SIZES[::-1]:
            check_same(gv.transform(pool[:n], 2), want[n], n)
        with pytest.raises(OrbfeError) as e:
            gv.transform(pool[:B.BOW_MAX + 1], 2)
        assert e.value.status == ORBFE_ERR_UNSUPPORTED
        check_same(gv.transform(pool[:65], 2), want[65], "after the refusal")
    finally:
        gv.close()


@pytest.mark.gpu
def test_gpu_sizes_batch(size_case):
    """cap = 4096 with slots of 0, 1, 1025 and 4096 features in one launch; cap = 4097 is refused."""
    from orbslam_mapsave_amd.abi import ORBFE_ERR_UNSUPPORTED
    from orbslam_mapsave_amd.native import OrbfeError
    case, pool, want = size_case
    gv = gpu_vocab(case)
    try:
        ns = (0, 1, 1025, 4096)
        for g, n in zip(batch_transform(gv, [pool[:n] for n in ns], B.BOW_MAX, 2), ns):
            check_same(g, want[n], n)
        with pytest.raises(OrbfeError) as e:
            batch_transform(gv, [pool[:1]], B.BOW_MAX + 1, 2)
        assert e.value.status == ORBFE_ERR_UNSUPPORTED
    finally:
        gv.close()


@pytest.mark.gpu
@pytest.mark.parametrize("opt", sorted(TEXT_OPTIONS))
def test_gpu_loader_agreement(opt, tmp_path):
    """orbfe_vocabulary_load_text and the oracle's loader on one file against the arrays
    constructor on the arrays the file was written from: info and a transform."""
    from orbslam_mapsave_amd.native import Vocabulary
    case = CASES["levelsup_ragged"]
    ov, path = oracle_vocab(case, tmp_path, **TEXT_OPTIONS[opt])
    ga = gpu_vocab(case)
    gt = Vocabulary(path, device=0)
    try:
        info = lambda v: (v.k, v.L, v.scoring, v.weighting, v.nodes, v.words)  # noqa: E731
        assert info(gt) == info(ga) == info(ov)
        want = B.transform(case["arrays"], 4, 0, 0, case["desc"], 2)
        for v in (gt, ga, ov):
            check_same(v.transform(case["desc"], 2), want, opt)
    finally:
        ga.close()
        gt.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(REFUSED))
def test_gpu_loaders_refuse(name, tmp_path):
    from orbslam_mapsave_amd.abi import ORBFE_ERR_ARG
    from orbslam_mapsave_amd.native import OrbfeError, Vocabulary
    k, L, sc, wt, arrays = REFUSED[name]()
    path = B.write_text(str(tmp_path / "bad.txt"), k, L, sc, wt, arrays)
    for load in (lambda: Vocabulary(path, device=0), lambda: oracle.Vocabulary(path)):
        with pytest.raises(OrbfeError) as e:
            load()
        assert e.value.status == ORBFE_ERR_ARG
    if name == "parent_is_self":
        with pytest.raises(OrbfeError) as e:
            Vocabulary.from_arrays(k, L, sc, wt, *arrays, device=0)
        assert e.value.status == ORBFE_ERR_ARG
