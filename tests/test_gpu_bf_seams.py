"""The FP4 brute-force matcher at the seams of its tiling, against the CPU oracle, exactly.

A workgroup is 4 waves x 64 queries (two 32-query halves per wave); references stream through
LDS in tiles of 64 rows (two 32-row m-tiles), and each reference fragment read from LDS serves
both query halves.  Reference counts sit on every m-tile and tile seam, query counts on every
half, wave and workgroup seam; ties sit across the m-tiles and tiles that the read order pairs;
the batched device call runs with the shared reference set pre-expanded or expanded by every
workgroup, and with per-entry reference sets.  Every case compares (best index, best distance,
second distance) with oracle.bf_match and requires equality.
"""
import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

NR = [1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257]
NQ = [1, 31, 32, 33, 63, 64, 65, 128, 255, 256, 257]


def _cross():
    """A sparse cross of NR x NQ: every value of either list meets a full partner (a multiple
    of 64) and a partial one of the other list."""
    full_q = [n for n in NQ if n % 64 == 0]
    part_q = [n for n in NQ if n % 64]
    full_r = [n for n in NR if n % 64 == 0]
    part_r = [n for n in NR if n % 64]
    pairs = []
    for i, nr in enumerate(NR):
        pairs += [(full_q[i % len(full_q)], nr), (part_q[i % len(part_q)], nr)]
    for i, nq in enumerate(NQ):
        pairs += [(nq, full_r[i % len(full_r)]), (nq, part_r[i % len(part_r)])]
    return sorted(set(pairs))


CROSS = _cross()


def test_cross_covers_both_lists():
    for nr in NR:
        assert any(r == nr and q % 64 == 0 for q, r in CROSS)
        assert any(r == nr and q % 64 for q, r in CROSS)
    for nq in NQ:
        assert any(q == nq and r % 64 == 0 for q, r in CROSS)
        assert any(q == nq and r % 64 for q, r in CROSS)


@pytest.fixture(scope="module")
def mt():
    from orbslam_mapsave_amd.native import ORBmatcher
    m = ORBmatcher(0.9, True, device=0)
    yield m
    m.close()


def _equal(got, exp):
    for g, e, name in zip(got, exp, ("best index", "best distance", "second distance")):
        assert np.array_equal(g, e), name


@pytest.mark.parametrize("nq,nr", CROSS)
def test_single_call_seams(mt, nq, nr):
    rng = np.random.default_rng(1000 * nq + nr)
    q = rng.integers(0, 256, (nq, 32), dtype=np.uint8)
    r = rng.integers(0, 256, (nr, 32), dtype=np.uint8)
    # near neighbours at the last row, and at the first row of the last m-tile, for some queries
    r[-1] = q[0]
    r[(nr - 1) // 32 * 32] = q[-1] ^ np.uint8(1)
    _equal(mt.bf_match(q, r), oracle.bf_match(q, r))


@pytest.mark.parametrize("delta", [32, 64, 128])
@pytest.mark.parametrize("k", [0, 31, 63])
def test_ties_across_read_order(mt, k, delta):
    """The same descriptor at reference rows k and k + delta: the lower index wins and the
    second distance equals the best, for a query at distance 0 and one a few bits away; the
    queries sit in both halves of a wave (rows i and i + 32 hold the same descriptor)."""
    rng = np.random.default_rng(64 * k + delta)
    r = rng.integers(0, 256, (200, 32), dtype=np.uint8)
    r[k + delta] = r[k]
    q = rng.integers(0, 256, (128, 32), dtype=np.uint8)
    near = r[k].copy()
    near[3] ^= 0x15  # 3 bits
    for i, d in ((5, r[k]), (70, near)):
        q[i] = q[i + 32] = d
    got = mt.bf_match(q, r)
    _equal(got, oracle.bf_match(q, r))
    for i, dist in ((5, 0), (37, 0), (70, 3), (102, 3)):
        assert got[0][i] == k and got[1][i] == dist and got[2][i] == dist, i


@pytest.mark.parametrize("lo,hi", [(10, 74), (62, 64), (40, 168)])
def test_nearest_pair_in_different_groups(mt, lo, hi):
    """A query whose two nearest references lie in different 64-row groups at distances 0 and 1,
    with the nearer one in the lower and in the higher group."""
    rng = np.random.default_rng(lo + hi)
    r = rng.integers(0, 256, (200, 32), dtype=np.uint8)
    q = rng.integers(0, 256, (70, 32), dtype=np.uint8)
    one = q[3].copy()
    one[31] ^= 0x80
    r[lo], r[hi] = q[3], one          # distance 0 below, 1 above
    other = q[40].copy()
    other[0] ^= 0x01
    r[lo + 1], r[hi + 1] = other, q[40]  # distance 1 below, 0 above
    got = mt.bf_match(q, r)
    _equal(got, oracle.bf_match(q, r))
    assert (got[0][3], got[1][3], got[2][3]) == (lo, 0, 1)
    assert (got[0][40], got[1][40], got[2][40]) == (hi + 1, 0, 1)


BATCH_NR = (129, 64, 0, 1)
BATCH_NQ = (65, 0, 33, 257)


@pytest.mark.parametrize("form", ["shared_pre", "shared_nopre", "per_entry"])
def test_batched_device_call(form, monkeypatch):
    """orbfe_bf_match_batch_device over four entries: one reference set for all (r_pitch 0),
    pre-expanded once per call or expanded by every workgroup, and a reference set per entry
    (r_pitch = cap * 32).  Rows past an entry's query count keep what the buffer held."""
    import torch
    from orbslam_mapsave_amd.native import ORBmatcher
    monkeypatch.setenv("ORBFE_BF_PRE", "0" if form == "shared_nopre" else "1")
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(5)
    nb, cap = len(BATCH_NR), 300
    rcap = cap  # per-entry reference sets in slabs of the queries' capacity, as config 4 holds them
    shared = form != "per_entry"
    ref = rng.integers(0, 256, (1 if shared else nb, rcap, 32), dtype=np.uint8)
    q = rng.integers(0, 256, (nb, cap, 32), dtype=np.uint8)
    ref[:, 70] = ref[:, 6]       # a tie across the two tiles: the lower row wins
    q[:, 2] = ref[0, 6]
    q[0, 64] = ref[0, 128]       # the last query of entry 0 meets the last reference
    d_r = torch.from_numpy(ref).to(dev)
    d_q = torch.from_numpy(q).to(dev)
    d_nq = torch.tensor(BATCH_NQ, dtype=torch.int32, device=dev)
    d_nr = torch.tensor(BATCH_NR, dtype=torch.int32, device=dev)
    d_out = torch.full((nb, cap, 3), -7, dtype=torch.int32, device=dev)
    mt = ORBmatcher(0.9, True, device=0)
    try:
        mt.bf_match_batch_device(d_q.data_ptr(), cap * 32, d_nq.data_ptr(), cap, d_r.data_ptr(),
                                 0 if shared else rcap * 32, d_nr.data_ptr(), nb, d_out.data_ptr())
        torch.cuda.synchronize()
        out = d_out.cpu().numpy()
    finally:
        mt.close()
    for b in range(nb):
        nq, nr = BATCH_NQ[b], BATCH_NR[b]
        assert (out[b, nq:] == -7).all(), b
        if nq == 0:
            continue
        exp = oracle.bf_match(q[b, :nq], ref[0 if shared else b, :nr])
        for c in range(3):
            assert np.array_equal(out[b, :nq, c], exp[c]), (b, c)
