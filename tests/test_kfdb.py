"""The keyframe database's restatement (tests/kfdb_cases.py) is a fit yardstick: its built cases
reach every branch, every single-decision mutant changes an answer on them, the scores depend on
the summation order and on the contraction where they should; and the library refuses bad
arguments without a device.  The comparison of the library with the restatement is in
tests/test_gpu_kfdb.py."""
import ctypes as C
import inspect
import re

import numpy as np
import pytest

import kfdb_cases as K
from orbslam_mapsave_amd import abi, native


@pytest.fixture(scope="module")
def baseline():
    stats = {}
    ans = {name: K.run_script(script, scoring, stats=stats)
           for name, scoring, script in K.built_scripts()}
    return ans, stats


def test_every_branch_is_reached(baseline):
    _, stats = baseline
    # every counter the restatement can emit.  The relocalisation form's second early return
    # (:335) has none: the keyframe of maxCommonWords always passes `words > minCommonWords`.
    expected = {"walk_first", "walk_again", "walk_connected", "walk_collision", "exit_no_sharing",
                "exit_no_scored", "words_pass", "words_fail", "words_equal_min", "score_pass",
                "score_fail", "score_equal_min", "neigh_absent", "neigh_skipped", "neigh_counted",
                "neigh_stale_score", "h18", "best_moves", "retain_pass", "retain_fail",
                "retain_equal", "duplicate_best"}
    emitted = set(re.findall(r'_bump\(st, "(\w+)"\)', inspect.getsource(K)))
    assert emitted == expected, emitted ^ expected
    assert set(stats) == expected, expected ^ set(stats)
    low = {k: v for k, v in stats.items() if v < 5}
    assert not low, low


@pytest.mark.parametrize("mutant", K.MUTANTS)
def test_every_mutant_changes_an_answer(mutant, baseline):
    ans, _ = baseline
    killed = [name for name, scoring, script in K.built_scripts()
              if K.run_script(script, scoring, mutant=mutant) != ans[name]]
    assert killed, mutant


def test_double_point_eight_is_not_a_mutant():
    """`maxCommonWords * 0.8f` (:195, :315) is a float product truncated to int.  A BowVector
    holds at most 4096 words, and for every such count the double product 0.8 truncates to the
    same int (the fractional part of m * 0.8 is a multiple of 0.2, far above either rounding), so
    "0.8 in place of 0.8f" cannot change an answer and is not among the mutants."""
    for m in range(0, 4097):
        assert int(np.float32(m) * np.float32(0.8)) == int(m * 0.8)


def test_built_cases_are_not_trivial(baseline):
    ans, _ = baseline
    t = ans["thresholds-0"]
    assert t[0][0] == ["A2", "A", "D", "B"]          # first word, then add sequence; C, G, E out
    assert t[1][0] == ["A2", "A", "D", "B"] and t[2][0] == ["A2", "A", "B"]
    states = t[2][2]
    assert states["C"][1] == 8 and states["C"][2] is None      # words == minCommonWords: unscored
    c = ans["covisibility-0"]
    assert c[0][0] == ["P"] and c[0][2]["CN"][:2] == (0, 1)    # connected: id not set, words end at 1
    assert c[0][2]["L"][2] is not None                         # below minScore, score still written
    s = ans["stale_scores-0"]
    assert s[4][1] and not s[1][1] and s[6][0] == ["U"]        # H18 only where nothing was written
    h = ans["collisions-0"]
    assert h[0][0] == [] and h[0][2]["A"][4] == 10 and h[2][2]["A"][1] == 20
    b = ans["all_below-0"]
    assert b[0][0] == [] and b[0][2]["A"][:2] == (70, 10) and b[0][2]["A"][2] is not None   # :216
    assert b[0][2]["C"][:3] == (70, 5, None) and b[0][2]["D"][:2] == (0, 1)
    assert b[1][0] == ["D"] and b[1][2]["A"][1] == 20 and b[2][0] == ["E"] and b[3][0] == []
    e = ans["erase_reuse-0"]
    assert e[1][0] == ["A", "E", "D"]                          # D sits in slot 1, last in add order
    n_queries = sum(len(a) for a in ans.values())
    n_nonempty = sum(1 for a in ans.values() for q in a if q[0])
    assert n_queries > 150 and n_nonempty > 100


@pytest.mark.parametrize("scoring", K.SCORINGS)
def test_score_depends_on_summation_order(scoring):
    i1, v1, i2, v2 = K.order_sensitive_pair(scoring)
    f = K.score(scoring, i1, v1, i2, v2, fused=False)
    assert f != K.score(scoring, i1, v1, i2, v2, fused=False, order="reverse")
    assert f != K.score(scoring, i1, v1, i2, v2, fused=False, order="pairwise")


@pytest.mark.parametrize("scoring", [1, 5])
def test_contraction_changes_l2_and_dot(scoring):
    i1, v1, i2, v2 = K.contraction_pair(scoring)
    assert K.score(scoring, i1, v1, i2, v2, True) != K.score(scoring, i1, v1, i2, v2, False)


@pytest.mark.parametrize("scoring", [0, 2, 4])
def test_contraction_leaves_the_other_scorings(scoring):
    i1, v1, i2, v2 = K.mixed_magnitude_pair()
    assert K.score(scoring, i1, v1, i2, v2, True) == K.score(scoring, i1, v1, i2, v2, False)


def test_score_formulas_on_known_values():
    ids = np.array([3, 7, 9], np.int32)
    a, b = np.array([0.5, 0.25, 0.25]), np.array([0.25, 0.5, 0.25])
    assert K.score(0, ids, a, ids, b) == 0.75                  # 1 - 0.5 * ||a - b||_1
    assert K.score(5, ids, a, ids, b) == 0.3125
    assert K.score(2, ids, a, ids, b) == 2.0 * (0.125 / 0.75 + 0.125 / 0.75 + 0.0625 / 0.5)
    assert K.score(1, ids, a * 4, ids, b * 4) == 1.0           # dot >= 1: clamped
    assert K.score(0, ids, a, ids + 100, b) == 0.0             # disjoint
    assert K.score(4, ids[:0], a[:0], ids, b) == 0.0           # empty


def test_seeded_scripts_run_and_collide():
    stats = {}
    out = K.run_script(K.seeded_script(1, 120), stats=stats)
    assert len(out) > 20 and stats.get("walk_collision", 0) > 0 and stats.get("retain_pass", 0) > 0


def test_bad_arguments_without_a_device():
    """Every entry point refuses a null handle (and what else can be judged without one) before
    it touches a device.  The refusals that need a live handle — nw > cap, unsorted ids, more
    than 10 neighbours, KL scoring, a freed slot — are in tests/test_gpu_kfdb.py: a vocabulary,
    and so a database, cannot be created without a device."""
    L = native.lib()
    ids = np.array([1, 2, 3], np.int32)
    vals = np.ones(3)
    slot, n, st = C.c_int32(0), C.c_int32(0), C.c_int(0)
    out = C.c_double(0)
    cand = np.zeros(8, np.int32)
    E = abi.ORBFE_ERR_ARG
    assert L.orbfe_vocabulary_set_arithmetic(None, 1) == E
    assert L.orbfe_vocabulary_score(None, abi.ptr(ids), abi.ptr(vals), 3, abi.ptr(ids),
                                    abi.ptr(vals), 3, C.byref(out)) == E
    assert L.orbfe_vocabulary_score_batch_device(None, 1, None, None, 8, None, None, None, None) == E
    assert not L.orbfe_kfdb_create(None, 64, 0, C.byref(st)) and st.value == E
    L.orbfe_kfdb_destroy(None)
    assert L.orbfe_kfdb_size(None) == E
    assert L.orbfe_kfdb_set_stream(None, None) == E
    assert L.orbfe_kfdb_add(None, abi.ptr(ids), abi.ptr(vals), 3, C.byref(slot)) == E
    assert L.orbfe_kfdb_add_device(None, None, None, None, C.byref(slot)) == E
    assert L.orbfe_kfdb_erase(None, 0) == E
    assert L.orbfe_kfdb_clear(None) == E
    assert L.orbfe_kfdb_set_covisibility(None, 0, 1, abi.ptr(cand)) == E
    assert L.orbfe_kfdb_set_scores(None, 0, 0.0, 0.0) == E
    assert L.orbfe_kfdb_get_state(None, 0, None) == E
    assert L.orbfe_kfdb_detect_loop_candidates(None, 1, abi.ptr(ids), abi.ptr(vals), 3, 0, None,
                                               0.0, abi.ptr(cand), 8, C.byref(n)) == E
    assert L.orbfe_kfdb_detect_relocalization_candidates(None, 1, abi.ptr(ids), abi.ptr(vals), 3,
                                                         abi.ptr(cand), 8, C.byref(n)) == E
    assert L.orbfe_kfdb_detect_loop_candidates_device(None, 1, None, None, None, 0, None, 0.0,
                                                      None, 0, C.byref(n)) == E
    assert L.orbfe_kfdb_detect_relocalization_candidates_device(None, 1, None, None, None, None,
                                                                0, C.byref(n)) == E
    assert C.sizeof(native.KfdbState) == 40
