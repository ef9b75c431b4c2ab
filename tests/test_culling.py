"""tests/culling_cases.py is not trivial: every mutant changes an answer on a built case, every
branch is taken, refusals change nothing, the shape scripts reach the sizes they are named after;
the decide / apply rounds the library runs for KeyFrameCulling equal the reference's sequential
loop on every built script and on 300 seeded dense maps; `10 r > 9 n` is the double comparison
through 8,192; and every new entry point refuses a null handle before it touches a device.  No GPU."""
import ctypes as C

import numpy as np

import culling_cases as Q
from orbslam_mapsave_amd import abi, native


def test_every_mutant_changes_an_answer():
    scripts = list(Q.built_scripts())
    base = {name: Q.run_script(s) for name, s in scripts}
    for mu in Q.MUTANTS:
        killed = [name for name, s in scripts if Q.run_script(s, mu) != base[name]]
        assert killed, mu


def test_every_branch_is_taken():
    st = {}
    for _, s in Q.built_scripts():
        Q.run_script(s, stats=st)
    for k in ("add_left_only", "add_present", "add_right", "badflag_empty", "badflag_observed",
              "cull_few_obs", "cull_kept", "cull_kept_inf", "cull_kept_nan", "cull_old", "cull_ratio",
              "cull_ratio_neg_inf", "cull_repeated", "cull_was_bad", "erase_absent", "erase_left_only",
              "erase_right", "erase_stays", "erase_to_bad", "match_is_point", "match_null",
              "match_other", "tracked_bad", "tracked_enough", "tracked_null", "tracked_too_few",
              "tracked_unchecked",
              "cull_after_a_cull", "cull_first_skipped", "dec_bad_point", "dec_cull", "dec_far",
              "dec_few_obs", "dec_held_twice", "dec_keep", "dec_nan_or_minus_zero", "dec_negative",
              "dec_no_points", "dec_not_redundant", "dec_octave_edge", "kfbad_deferred", "kfbad_first",
              "kfbad_left_only", "kfbad_no_parent", "kfbad_not_listed", "kfbad_point_bad",
              "kfbad_point_stays", "kfbad_right", "kfbad_second_index", "seterase_plain",
              "seterase_runs", "tree_bad_child", "tree_leftover", "tree_leftover_bad",
              "tree_listed_without_weight", "tree_no_candidate", "tree_orphan", "tree_reassigned"):
        assert st.get(k, 0) >= 5, (k, st.get(k, 0))


def test_refusals_change_nothing():
    n = 0
    for _, s in Q.built_scripts():
        m = Q.Model()
        for op in s:
            before = m.state() if op[0] in Q.OPS else None
            a = m.run(op)
            if isinstance(a, tuple) and a[0] == "error":
                assert a[1] == before, op
                n += 1
    assert n >= 30


def _rounds_equal_the_loop(script):
    """Every cullkfs of the script, run as the sequential loop on one model and as decide / apply
    rounds on a copy -> (calls, calls that culled two or more, the most rounds of one call)."""
    import copy
    m = Q.Model()
    calls = multi = most = 0
    for op in script:
        if op[0] != "cullkfs":
            m.run(op)
            continue
        m2 = copy.deepcopy(m)
        want = m.run(op)
        if want[0] in ("error", "capacity"):
            continue
        got, rounds = m2.cull_keyframes_rounds(op[1], op[2], op[3], op[4])
        assert (got, m2.state()) == want, op
        n = sum(1 for x in want[0][1] if x == Q.CULLED)
        assert rounds <= n + 1
        calls += 1
        multi += n >= 2
        most = max(most, rounds)
    return calls, multi, most


def test_rounds_equal_the_sequential_loop_on_built_scripts():
    calls = 0
    for _, s in Q.built_scripts():
        calls += _rounds_equal_the_loop(s)[0]
    assert calls >= 30


def test_rounds_equal_the_sequential_loop_on_seeded_maps():
    multi = most = 0
    for seed in range(300):
        c, m, r = _rounds_equal_the_loop(Q.seeded_kf_script(seed))
        multi += m > 0
        most = max(most, r)
    assert multi >= 50 and most >= 3, (multi, most)


def test_sequencing_matters_on_seeded_maps():
    """Deciding every keyframe at once on the unchanged map is a different function."""
    n = sum(Q.run_script(Q.seeded_kf_script(seed), "one_shot") != Q.run_script(Q.seeded_kf_script(seed))
            for seed in range(60))
    assert n >= 20


def test_the_integer_form_of_the_threshold():
    """nRedundantObservations > 0.9 * nMPs (int against double) is 10 r > 9 n for every
    0 <= r <= n <= 8192."""
    for n in range(8193):
        r = np.arange(n + 1)
        assert np.array_equal(r > 0.9 * n, 10 * r > 9 * n), n


def test_the_found_ratio_is_a_float_division():
    """2^24 / (2^26 + 1): exactly 0.25 in float (kept), below it in double."""
    m = Q.Model()
    m.apply(("points", ["p"]))
    m.mps["p"].found, m.mps["p"].visible = 1 << 24, (1 << 26) + 1
    assert m.found_ratio("p") == np.float32(0.25) and m.found_ratio("p", "ratio_double") < 0.25
    assert m.cull_points(["p"], 0, True) == (["p"], [])


def test_shape_scripts_hit_their_sizes():
    a = Q.run_script(Q.script_observation_rows())
    sizes = (0, 1, 2, 3, 4, 63, 64, 65, 200)
    before = a[-4][1][1]            # after the obsidx
    assert [len(before[f"r{n}"][1]) for n in sizes] == list(sizes)
    assert [len(before[f"c{n}"][1]) for n in sizes] == list(sizes)
    after = a[-1][1]
    assert a[-1][0] == ([], [f"c{n}" for n in sizes])
    assert all(after[1][f"{t}{n}"][:2] == (True, []) for n in sizes for t in "rc")
    held = sum(1 for mps, *_ in after[0].values() for p in mps if p is not None)
    assert held == sum(1 for mps, *_ in a[-4][1][0].values() for p in mps if p is not None) - 2 * sum(sizes)
    a = Q.run_script(Q.script_keyframe_slots())
    assert [len(a[-1][1][0][f"S{n}"][0]) for n in (0, 1, 63, 64, 65, 1024, 1025, 8192)] == \
        [0, 1, 63, 64, 65, 1024, 1025, 8192]
    assert a[-1][0] == a[-5][0] - 1 > 5000
    for n in (0, 1, 64, 65, 257, 1025):
        out = Q.run_script(Q.script_cull_list(n))[-1][0]
        assert len(out[0]) + len(out[1]) <= n and (n < 63 or (out[0] and out[1]))


def test_null_handles_and_bad_arguments_without_a_device():
    L = native.lib()
    E = abi.ORBFE_ERR_ARG
    a = np.zeros(8, np.int32)
    u = np.ones(8, np.uint8)
    f = np.zeros(8, np.float32)
    k = np.zeros(8, np.int64)
    n, m = C.c_int32(0), C.c_int32(0)
    th = C.c_float(0)
    p = abi.ptr
    assert L.orbfe_map_set_keyframe_features(None, 0, 8, p(a), p(f), p(f), 1.0) == E
    assert L.orbfe_map_get_keyframe_features(None, 0, 8, p(a), p(u), p(f), C.byref(th), C.byref(n)) == E
    assert L.orbfe_map_add_observations_idx(None, 8, p(a), p(a), p(a)) == E
    assert L.orbfe_map_add_observations_idx(None, 0, None, None, None) == E
    assert L.orbfe_map_erase_observation(None, 0, 0, C.byref(n)) == E
    assert L.orbfe_map_set_point_bad_flag(None, 8, p(a)) == E
    assert L.orbfe_map_set_point_bad_flag(None, 0, None) == E
    assert L.orbfe_map_set_point_counters(None, 8, p(a), p(a), p(a), p(a), p(k)) == E
    assert L.orbfe_map_get_point_counters(None, 8, p(a), p(a), p(a), p(a), p(k)) == E
    assert L.orbfe_map_increase_counters(None, native.MAP_FOUND, 8, p(a), None) == E
    assert L.orbfe_map_increase_counters_device(None, native.MAP_VISIBLE, 8, p(a), None) == E
    assert L.orbfe_map_cull_points(None, 5, 0, p(a), 8, C.byref(n), p(a), C.byref(m)) == E
    assert L.orbfe_map_tracked_map_points(None, 0, 1, C.byref(n)) == E
    assert L.orbfe_map_get_keyframe_points(None, 0, p(a), 8, C.byref(n)) == E
    assert L.orbfe_map_get_observations(None, 0, p(a), p(a), 8, C.byref(n)) == E
    assert L.orbfe_map_get_bad_flags(None, 0, 8, p(a), p(u)) == E
    assert L.orbfe_map_set_not_erase(None, 0, 1) == E
    assert L.orbfe_map_get_erase_flags(None, 0, C.byref(n), C.byref(m)) == E
    w = C.c_int32(0)
    assert L.orbfe_map_set_keyframe_bad_flag(None, 0, 0, C.byref(w), p(a), 8, C.byref(n), p(a), 4, C.byref(m)) == E
    assert L.orbfe_map_set_erase(None, 0, 0, 0, C.byref(w), p(a), 8, C.byref(n), p(a), 4, C.byref(m)) == E
    assert L.orbfe_map_cull_keyframes(None, 0, 2, p(a), -1, 0, p(a), 8, C.byref(w), p(a), 8, C.byref(n),
                                      p(a), 4, C.byref(m)) == E
    assert L.orbfe_map_cull_keyframes(None, 0, -1, None, -1, 0, None, 0, C.byref(w), None, 0, None,
                                      None, 0, None) == E
