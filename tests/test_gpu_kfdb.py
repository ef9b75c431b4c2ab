"""ORBVocabulary::score and the keyframe database on the device against the restatement of
tests/kfdb_cases.py: bit-exact double scores for the five scoring kinds (host form and batch
device form), every built case and seeded sequences of adds, erases and queries (candidate list
with its order, status and all six state fields of every keyframe after every call), the host
forms against the _device forms, the 4096-entry limit, the refusals that need a handle, and the
chain transform batch -> add_device -> relocalisation query -> SearchByBoW batch."""
import ctypes as C

import numpy as np
import pytest

import kfdb_cases as K
import scenarios as S
from orbslam_mapsave_amd import abi
from orbslam_mapsave_amd.synth import synthetic_vocabulary_text

pytestmark = pytest.mark.gpu

UNSUPPORTED = abi.ORBFE_ERR_UNSUPPORTED


@pytest.fixture(scope="module")
def vocabs(tmp_path_factory):
    """One 8^4 = 4096-word vocabulary per scoring kind (KL included, for the refusal)."""
    from orbslam_mapsave_amd.native import Vocabulary
    d = tmp_path_factory.mktemp("kfdb_voc")
    out = {}
    for sc in (0, 1, 2, 3, 4, 5):
        p = str(d / ("voc%d.txt" % sc))
        synthetic_vocabulary_text(p, 8, 4, seed=3, scoring=sc, weighting=0)
        out[sc] = Vocabulary(p, device=0)
    yield out
    for v in out.values():
        v.close()


def bits(x):
    return np.array(x, np.float64).view(np.uint64)


# ---- scores ------------------------------------------------------------------------------------

def score_pairs(scoring):
    rng = np.random.Generator(np.random.PCG64(40 + scoring))
    pairs = []
    e = (np.zeros(0, np.int32), np.zeros(0))
    a = K.random_bow(rng, 4096, 50)
    pairs += [(*e, *e), (*e, *a), (*a, *e)]
    pairs.append((*K.random_bow(rng, 2000, 40), *K.random_bow(rng, 4096, 40, lo=2000)))  # disjoint
    for n in (1, 63, 64, 65, 4096):
        i1, v1 = K.random_bow(rng, 4096, n)
        pairs.append((i1, v1, i1.copy(), rng.uniform(0.01, 1.0, n) / n))
        pairs.append((*K.random_bow(rng, 4096, max(n // 2, 1)), *K.random_bow(rng, 4096, n)))
    pairs.append(K.order_sensitive_pair(scoring))
    if scoring in (1, 5):
        pairs.append(K.contraction_pair(scoring))
    z = np.array([5, 9], np.int32)
    pairs.append((z, np.array([0.0, 0.5]), z, np.array([0.0, 0.25])))  # chi-square's 0 + 0 guard
    return pairs


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("scoring", K.SCORINGS)
def test_scores(scoring, fused, vocabs):
    import torch
    v = vocabs[scoring]
    v.set_arithmetic(1 if fused else 0)
    pairs = score_pairs(scoring)
    want = [K.score(scoring, *p, fused=fused) for p in pairs]
    got = [v.score(*p) for p in pairs]
    for p, (w, g) in enumerate(zip(want, got)):
        assert bits(w) == bits(g), (p, w, g)
    # the same vectors as slots 2p, 2p + 1 of a transform batch's layout
    cap, n = 4096, 2 * len(pairs)
    ids = np.zeros((n, cap), np.int32)
    vals = np.zeros((n, cap), np.float64)
    nw = np.zeros(n, np.int32)
    for p, (i1, v1, i2, v2) in enumerate(pairs):
        for s, (i, x) in ((2 * p, (i1, v1)), (2 * p + 1, (i2, v2))):
            ids[s, :len(i)], vals[s, :len(i)], nw[s] = i, x, len(i)
    dev = torch.device("cuda", 0)
    D = [torch.from_numpy(x).to(dev) for x in (ids, vals, nw)]
    pa = torch.arange(0, n, 2, dtype=torch.int32, device=dev)
    pb = pa + 1
    out = torch.full((len(pairs),), -7.0, dtype=torch.float64, device=dev)
    v.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    v.score_batch_device(len(pairs), pa.data_ptr(), pb.data_ptr(), cap, D[0].data_ptr(),
                         D[1].data_ptr(), D[2].data_ptr(), out.data_ptr())
    torch.cuda.synchronize()
    v.set_stream(None)
    v.set_arithmetic(1)
    assert np.array_equal(bits(out.cpu().numpy()), bits(want))
    if scoring in (1, 5):  # the two readings differ on the pair built for it
        i = len(pairs) - 2
        assert bits(K.score(scoring, *pairs[i], fused=True)) != bits(K.score(scoring, *pairs[i], fused=False))


# ---- queries -----------------------------------------------------------------------------------

class Runner:
    """Runs a script of kfdb_cases on a library database; host forms or _device forms."""

    def __init__(self, voc, cap, device=False, slots_hint=0):
        from orbslam_mapsave_amd.native import KeyFrameDatabase
        self.db = KeyFrameDatabase(voc, cap, slots_hint)
        self.device = device
        self.slot, self.name = {}, {}

    def states(self):
        out = {}
        for name, s in self.slot.items():
            st = self.db.get_state(s)
            f = lambda x: int(np.array(x, np.float32).view(np.uint32))
            out[name] = (st.loop_query, st.loop_words, f(st.loop_score) if st.scores_set & 1 else None,
                         st.reloc_query, st.reloc_words, f(st.reloc_score) if st.scores_set & 2 else None)
        return out

    def query(self, loop, qid, ids, vals, conn=(), min_score=0.0):
        conn = [self.slot[c] for c in conn if c in self.slot]
        if not self.device:
            if loop:
                return self.db.DetectLoopCandidates(qid, ids, vals, conn, min_score)
            return self.db.DetectRelocalizationCandidates(qid, ids, vals)
        import torch
        dev = torch.device("cuda", 0)
        i = torch.from_numpy(np.ascontiguousarray(ids, np.int32)).to(dev)
        v = torch.from_numpy(np.ascontiguousarray(vals, np.float64)).to(dev)
        n = torch.tensor([len(ids)], dtype=torch.int32, device=dev)
        c = torch.tensor(conn + [0], dtype=torch.int32, device=dev)
        cand = torch.full((4096,), -9, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        if loop:
            nc, st = self.db.detect_loop_candidates_device(
                qid, i.data_ptr(), v.data_ptr(), n.data_ptr(), len(conn), c.data_ptr(), min_score,
                cand.data_ptr(), 4096)
        else:
            nc, st = self.db.detect_relocalization_candidates_device(
                qid, i.data_ptr(), v.data_ptr(), n.data_ptr(), cand.data_ptr(), 4096)
        got = cand.cpu().numpy()
        assert (got[nc:] == -9).all()
        return got[:nc], st

    def run(self, script):
        out = []
        for op in script:
            if op[0] == "add":
                s = self.db.add(op[2], op[3])
                assert s not in self.name
                self.slot[op[1]], self.name[s] = s, op[1]
            elif op[0] == "erase":
                s = self.slot.pop(op[1])
                del self.name[s]
                self.db.erase(s)
            elif op[0] == "clear":
                self.db.clear()
                self.slot, self.name = {}, {}
            elif op[0] == "covis":
                self.db.set_covisibility(self.slot[op[1]],
                                         [-1 if n is None else self.slot[n] for n in op[2]])
            elif op[0] == "scores":
                self.db.set_scores(self.slot[op[1]], op[2], op[3])
            else:
                cand, st = self.query(op[0] == "loop", *op[1:])
                out.append(([self.name[int(s)] for s in cand], st == UNSUPPORTED, self.states()))
            assert len(self.db) == len(self.slot)
        return out


def check(got, want):
    assert len(got) == len(want)
    for q, (g, w) in enumerate(zip(got, want)):
        assert g[0] == w[0], ("candidates", q, g[0], w[0])
        assert g[1] == w[1], ("status", q)
        assert g[2] == w[2], ("state", q, {k: (g[2][k], w[2][k]) for k in w[2] if g[2].get(k) != w[2][k]})


BUILT = {name: (scoring, script) for name, scoring, script in K.built_scripts()}


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("name", sorted(BUILT))
def test_built_cases(name, device, vocabs):
    scoring, script = BUILT[name]
    want = K.run_script(script, scoring)
    r = Runner(vocabs[scoring], 64, device)
    check(r.run(script), want)
    r.db.close()


@pytest.mark.parametrize("size,ops,device", [(0, 150, False), (1, 150, True), (64, 120, False),
                                             (257, 60, True), (2000, 24, False)])
@pytest.mark.parametrize("scoring", [0, 1])
def test_seeded_sequences(size, ops, device, scoring, vocabs):
    """Databases of 0, 1, 64, 257 and about 2000 keyframes; the storage (16 slots at first)
    doubles in the middle of the sequences; query ids repeat (H19)."""
    script = K.seeded_script(size + scoring, ops, nkf0=size)
    stats = {}
    want = K.run_script(script, scoring, stats=stats)
    r = Runner(vocabs[scoring], 40, device)
    check(r.run(script), want)
    r.db.close()
    assert len(want) > 3 and stats.get("walk_first", 0) > 0


@pytest.mark.parametrize("n", [4096, 4097])
def test_entry_limit(n, vocabs):
    """Every keyframe identical to the query: all of them are scored.  4096 entries are exact
    (add order), 4097 exceed the tail's sort and return ORBFE_ERR_CAPACITY."""
    from orbslam_mapsave_amd.native import OrbfeError
    ids = np.array([3, 10, 11, 400, 2000], np.int32)
    vals = np.array([0.5, 0.125, 0.125, 0.125, 0.125])
    r = Runner(vocabs[0], 8, slots_hint=n)
    for i in range(n):
        r.db.add(ids, vals)
    if n > 4096:
        with pytest.raises(OrbfeError) as e:
            r.db.DetectRelocalizationCandidates(9, ids, vals)
        assert e.value.status == abi.ORBFE_ERR_CAPACITY
    else:
        cand, st = r.db.DetectRelocalizationCandidates(9, ids, vals)
        assert st == 0 and np.array_equal(cand, np.arange(n))
        cand, st = r.db.DetectLoopCandidates(9, ids, vals, [5, 77], 1.0)
        assert st == 0 and np.array_equal(cand, [i for i in range(n) if i not in (5, 77)])
        one = int(np.array(1.0, np.float32).view(np.uint32))
        for s in (0, 5, 77, 4095):
            t = r.db.get_state(s)
            conn = s in (5, 77)
            assert (t.reloc_query, t.reloc_words, t.scores_set & 2) == (9, 5, 2)
            assert (t.loop_query, t.loop_words, t.scores_set & 1) == ((0, 1, 0) if conn else (9, 5, 1))
            assert int(np.array(t.reloc_score, np.float32).view(np.uint32)) == one
    r.db.close()


def test_refusals(vocabs):
    from orbslam_mapsave_amd.native import KeyFrameDatabase, OrbfeError, lib
    import torch
    L = lib()
    E = abi.ORBFE_ERR_ARG
    v = vocabs[0]
    st = C.c_int(0)
    assert not L.orbfe_kfdb_create(v._h, 4097, 0, C.byref(st)) and st.value == E
    db = KeyFrameDatabase(v, 8)
    ids = np.arange(9, dtype=np.int32)
    vals = np.ones(9)
    slot, n = C.c_int32(-1), C.c_int32(0)
    cand = np.zeros(4, np.int32)
    p = abi.ptr
    assert L.orbfe_kfdb_add(db._h, p(ids), p(vals), 9, C.byref(slot)) == E           # nw > cap
    bad = np.array([4, 4, 9], np.int32)
    assert L.orbfe_kfdb_add(db._h, p(bad), p(vals), 3, C.byref(slot)) == E           # not ascending
    big = np.array([1, 4096], np.int32)
    assert L.orbfe_kfdb_add(db._h, p(big), p(vals), 2, C.byref(slot)) == E           # word >= nwords
    assert L.orbfe_kfdb_detect_relocalization_candidates(db._h, 1, p(bad), p(vals), 3, p(cand), 4,
                                                         C.byref(n)) == E
    assert L.orbfe_kfdb_detect_relocalization_candidates(db._h, 1, p(ids), p(vals), 9, p(cand), 4,
                                                         C.byref(n)) == E
    assert len(db) == 0
    a, b = db.add(ids[:5], vals[:5]), db.add(ids[:4], vals[:4])
    assert (a, b) == (0, 1)
    assert L.orbfe_kfdb_set_covisibility(db._h, a, 11, p(np.zeros(11, np.int32))) == E
    db.erase(b)
    assert L.orbfe_kfdb_erase(db._h, b) == E                                         # freed slot
    assert L.orbfe_kfdb_get_state(db._h, b, C.byref(abi_state())) == E
    assert L.orbfe_kfdb_set_scores(db._h, b, 0.0, 0.0) == E
    assert L.orbfe_kfdb_set_covisibility(db._h, a, 1, p(np.array([b], np.int32))) == E
    assert L.orbfe_kfdb_set_covisibility(db._h, 7, 0, None) == E
    # add_device validates on the device; a refused vector does not take the slot
    dev = torch.device("cuda", 0)
    di = torch.tensor([4, 4, 9], dtype=torch.int32, device=dev)
    dv = torch.ones(3, dtype=torch.float64, device=dev)
    dn = torch.tensor([3], dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    assert L.orbfe_kfdb_add_device(db._h, di.data_ptr(), dv.data_ptr(), dn.data_ptr(), C.byref(slot)) == E
    dn9 = torch.tensor([9], dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    assert L.orbfe_kfdb_add_device(db._h, di.data_ptr(), dv.data_ptr(), dn9.data_ptr(), C.byref(slot)) == E
    assert len(db) == 1 and db.add(ids[:3], vals[:3]) == b
    # the _device forms validate the query on the device, before any state is touched: a count
    # above the database's cap (a transform batch with a larger cap), a negative one, unsorted ids
    qi = torch.tensor([0, 1, 2, 3, 4, 5, 6, 7, 8], dtype=torch.int32, device=dev)
    qv = torch.ones(9, dtype=torch.float64, device=dev)
    dc = torch.full((4,), -9, dtype=torch.int32, device=dev)
    before = bytes(db.get_state(a))
    for cnt, ids_t in ((9, qi), (-1, qi), (3, di)):
        dq = torch.tensor([cnt], dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        n.value = 7
        assert L.orbfe_kfdb_detect_relocalization_candidates_device(
            db._h, 41, ids_t.data_ptr(), qv.data_ptr(), dq.data_ptr(), dc.data_ptr(), 4, C.byref(n)) == E
        assert L.orbfe_kfdb_detect_loop_candidates_device(
            db._h, 41, ids_t.data_ptr(), qv.data_ptr(), dq.data_ptr(), 0, None, 0.0, dc.data_ptr(), 4,
            C.byref(n)) == E
        assert n.value == 0 and bytes(db.get_state(a)) == before and (dc.cpu().numpy() == -9).all()
    dq = torch.tensor([8], dtype=torch.int32, device=dev)   # and the same vector within cap is fine
    torch.cuda.synchronize()
    assert L.orbfe_kfdb_detect_relocalization_candidates_device(
        db._h, 41, qi.data_ptr(), qv.data_ptr(), dq.data_ptr(), dc.data_ptr(), 4, C.byref(n)) == 0
    assert n.value == 1 and int(dc[0]) == a and db.get_state(a).reloc_query == 41
    # a candidate buffer that is too small: the count comes back
    assert L.orbfe_kfdb_detect_relocalization_candidates(db._h, 5, p(ids[:5]), p(vals[:5]), 5,
                                                         p(cand), 0, C.byref(n)) == abi.ORBFE_ERR_CAPACITY
    assert n.value == 1
    db.close()
    # KL scoring
    kl = vocabs[3]
    with pytest.raises(OrbfeError) as e:
        kl.score(ids[:3], vals[:3], ids[:3], vals[:3])
    assert e.value.status == UNSUPPORTED
    db = KeyFrameDatabase(kl, 8)
    db.add(ids[:3], vals[:3])
    assert L.orbfe_kfdb_detect_relocalization_candidates(db._h, 5, p(ids[:3]), p(vals[:3]), 3,
                                                         p(cand), 4, C.byref(n)) == UNSUPPORTED
    db.close()


def abi_state():
    from orbslam_mapsave_amd.native import KfdbState
    return KfdbState()


# ---- the chain on the device -------------------------------------------------------------------

def test_transform_to_candidates_to_search_by_bow(vocabs):
    """transform batch -> add_device -> relocalisation query (device form) -> its candidates as the
    pair list of orbfe_search_by_bow_batch_device, with no BowVector or candidate crossing to the
    host; against the same chain through the host forms (orbfe_bow_transform, orbfe_kfdb_add, the
    host query, orbfe_search_by_bow per candidate).  The batch scores of the same slots too."""
    import torch
    from orbslam_mapsave_amd.native import KeyFrameDatabase, ORBmatcher
    v = vocabs[0]
    rng = np.random.Generator(np.random.PCG64(5))
    frames = [S.extract_frame(s, 600, ini=20) for s in (0, 1, 2)]
    frames += [S.extract_frame(0, 600, shift=(-4, 5), ini=20), S.extract_frame(0, 600, shift=(2, -3), ini=20)]
    nf, q = len(frames), len(frames) - 1       # the last frame is the query; the others keyframes
    cap = 700
    dev = torch.device("cuda", 0)
    d = np.zeros((nf, cap, 32), np.uint8)
    ang = np.zeros((nf, cap), np.float32)
    ok = np.zeros((nf, cap), np.uint8)
    for i, f in enumerate(frames):
        d[i, :f.n], ang[i, :f.n] = f.desc, f.keys["angle"]
        ok[i, :f.n] = rng.uniform(size=f.n) < 0.8
    D, A, OK = (torch.from_numpy(x).to(dev) for x in (d, ang, ok))
    N = torch.tensor([f.n for f in frames], dtype=torch.int32, device=dev)
    wid = torch.zeros((nf, cap), dtype=torch.int32, device=dev)
    val = torch.zeros((nf, cap), dtype=torch.float64, device=dev)
    nid = torch.zeros((nf, cap), dtype=torch.int32, device=dev)
    off = torch.zeros((nf, cap + 1), dtype=torch.int32, device=dev)
    feat = torch.zeros((nf, cap), dtype=torch.int32, device=dev)
    nw = torch.zeros(nf, dtype=torch.int32, device=dev)
    nn = torch.zeros(nf, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    v.set_stream(stream)
    v.transform_batch_device(nf, D.data_ptr(), N.data_ptr(), cap, 2, wid.data_ptr(), val.data_ptr(),
                             nw.data_ptr(), nid.data_ptr(), off.data_ptr(), feat.data_ptr(), nn.data_ptr())
    pa = torch.tensor([q] * q, dtype=torch.int32, device=dev)
    pb = torch.arange(q, dtype=torch.int32, device=dev)
    sc = torch.zeros(q, dtype=torch.float64, device=dev)
    v.score_batch_device(q, pa.data_ptr(), pb.data_ptr(), cap, wid.data_ptr(), val.data_ptr(),
                         nw.data_ptr(), sc.data_ptr())
    torch.cuda.synchronize()
    v.set_stream(None)
    db = KeyFrameDatabase(v, cap)
    db.set_stream(stream)
    for i in range(q):      # slot i = batch slot i: the candidates index the batch directly
        assert db.add_device(wid[i].data_ptr(), val[i].data_ptr(), nw[i:].data_ptr()) == i
    db.set_covisibility(0, [3])
    cand = torch.full((q,), -1, dtype=torch.int32, device=dev)
    nc, st = db.detect_relocalization_candidates_device(77, wid[q].data_ptr(), val[q].data_ptr(),
                                                        nw[q:].data_ptr(), cand.data_ptr(), q)
    assert st == 0 and nc >= 1
    pf = torch.full((nc,), q, dtype=torch.int32, device=dev)
    out = torch.full((nc, cap), 7, dtype=torch.int32, device=dev)
    nm = torch.zeros(nc, dtype=torch.int32, device=dev)
    ms = torch.full((1,), 9, dtype=torch.int32, device=dev)
    mt = ORBmatcher(0.75, True, device=0)
    mt.set_stream(stream)
    mt.search_by_bow_batch_device(
        nc, cand.data_ptr(), pf.data_ptr(), cap, D.data_ptr(), A.data_ptr(), OK.data_ptr(),
        nn.data_ptr(), nid.data_ptr(), off.data_ptr(), feat.data_ptr(), cap, D.data_ptr(),
        A.data_ptr(), nn.data_ptr(), nid.data_ptr(), off.data_ptr(), feat.data_ptr(),
        out.data_ptr(), nm.data_ptr(), ms.data_ptr())
    torch.cuda.synchronize()
    assert int(ms[0]) == 0
    # the host chain
    tr = [v.transform(f.desc, 2) for f in frames]
    hdb = KeyFrameDatabase(v, cap)
    for i in range(q):
        assert hdb.add(tr[i][0], tr[i][1]) == i
    hdb.set_covisibility(0, [3])
    hcand, hst = hdb.DetectRelocalizationCandidates(77, tr[q][0], tr[q][1])
    assert hst == 0 and np.array_equal(hcand, cand.cpu().numpy()[:nc])
    for i in range(q):
        assert bits(sc[i].item()) == bits(v.score(tr[q][0], tr[q][1], tr[i][0], tr[i][1]))
        assert bits(sc[i].item()) == bits(K.score(0, tr[q][0], tr[q][1], tr[i][0], tr[i][1]))
    hm = ORBmatcher(0.75, True, device=0)
    got, gnm = out.cpu().numpy(), nm.cpu().numpy()
    fq = frames[q]
    for p, k in enumerate(hcand):
        m, n = hm.SearchByBoW(frames[k].desc, frames[k].keys["angle"], ok[k, :frames[k].n],
                              tr[k][2:], fq.desc, fq.keys["angle"], tr[q][2:])
        assert n == gnm[p] and np.array_equal(m, got[p, :fq.n])
    assert gnm.max() > 20
    # and against the restatement
    rdb = K.DB(0)
    for i in range(q):
        rdb.add("k%d" % i, tr[i][0], tr[i][1])
    rdb.covis("k0", ["k3"])
    rc, _ = rdb.detect_reloc(77, tr[q][0], tr[q][1])
    assert rc == ["k%d" % k for k in hcand]
    for x in (db, hdb, mt, hm):
        x.close()
