"""The covisibility graph's restatement (tests/covis_cases.py) is a fit yardstick: its built cases
reach every branch, every single-decision mutant changes an answer on them, they are not trivial,
and the closed form of a sequential batch equals the literal loop; and the library refuses null
handles without a device.  The comparison of the library with the restatement is in
tests/test_gpu_covis.py."""
import ctypes as C
import inspect
import re

import numpy as np
import pytest

import covis_cases as K
from orbslam_mapsave_amd import abi, native


@pytest.fixture(scope="module")
def baseline():
    stats = {}
    ans = {name: K.run_script(script, stats=stats) for name, script in K.built_scripts()}
    return ans, stats


def test_every_branch_is_reached(baseline):
    _, stats = baseline
    src = inspect.getsource(K.Model)
    emitted = set(re.findall(r'_bump\(st, "(\w+)"', src)) | {"best_sub_threshold", "best_all_over",
                                                              "max_new", "over_th", "at_th"}
    emitted -= {"max_mutant"}    # reached by the mutant max_ge only
    assert set(stats) == emitted, emitted ^ set(stats)
    low = {k: v for k, v in stats.items() if v < 5}
    assert not low, low


def test_required_mutants_are_present():
    required = {"self_counted", "bad_point_counted", "dup_point_once", "th_gt", "max_ge",
                "max_always_added", "weights_thresholded", "ordered_full", "tie_ascending_key",
                "order_ascending", "parent_every_time", "parent_for_id0", "parent_back",
                "first_flag_kept", "empty_clears", "neighbour_not_told", "add_same_weight_resorts",
                "add_never_resorts", "resort_thresholded", "erase_absent_resorts",
                "erasekf_keeps_own", "by_weight_all"}
    assert required <= set(K.MUTANTS) and len(K.MUTANTS) == len(set(K.MUTANTS))
    src = inspect.getsource(K.Model)
    for m in K.MUTANTS:
        assert f'"{m}"' in src, m


@pytest.mark.parametrize("mutant", K.MUTANTS)
def test_every_mutant_changes_an_answer(mutant, baseline):
    ans, _ = baseline
    killed = [name for name, script in K.built_scripts()
              if K.run_script(script, mutant=mutant) != ans[name]]
    assert killed, mutant


def test_built_cases_are_not_trivial(baseline):
    ans, _ = baseline
    t = ans["threshold-0"]
    # keys run against the slots in variant 0, so E < D < C < B by key.  A counts B 14, C 15, D 16,
    # E 15: B is below the threshold and stays in the weight map only; C and E tie at 15 and the
    # higher key (C) comes first
    g = t[0]
    assert g["A"][1] == [("D", 16), ("C", 15), ("E", 15)]
    assert g["A"][0] == [("E", 15), ("D", 16), ("C", 15), ("B", 14)]
    assert g["A"][2] == "D" and g["D"][3] == ["A"] and g["A"][4] is False
    assert g["C"][0] == [("A", 15)] and g["C"][1] == [("A", 15)] and g["B"][0] == []   # B was not told
    g = t[1]                                                      # B: only A at 14, the max rule
    assert g["B"][1] == [("A", 14)] and g["A"][0][-1] == ("B", 14) and g["A"][1] == t[0]["A"][1]
    g = t[3]                                                      # H: I and J tie at 3, K has 2: the lowest key
    assert g["H"][1] == [("J", 3)] and g["H"][2] == "J" and g["H"][0] == [("K", 2), ("J", 3), ("I", 3)]
    g = ans["threshold-1"][3]                                     # three tied at 4
    assert [w for _, w in g["H"][0]] == [4, 4, 4] and g["H"][1] == [g["H"][0][0]]
    assert t[4] == t[3]                                           # Z holds nothing: nothing changes
    assert t[5][1] == [] and t[6][1] == ["D"] and t[7][1] == [] and t[8][1] == []   # the it == end quirk
    a = ans["addconn-0"]
    assert a[1] == a[0] and a[2] == a[0]                          # equal weight, absent erase
    assert a[0]["A"][1] == [("B", 17), ("C", 15)]
    assert a[5]["A"][1] == [("B", 18), ("C", 15), ("D", 9), ("E", 4)]   # changed: the full sort
    assert a[6]["A"][1] == [("B", 17), ("C", 15)] and a[6]["B"][1] == a[0]["B"][1]
    y = ans["asymmetric-0"]
    assert y[0]["B"][1] == [("C", 15)]
    assert y[1]["B"][1] == [("A", 21), ("C", 15), ("D", 6)]       # told 21 where it held 5
    assert y[3]["B"][1] == [("C", 15)]                            # A before B: B's own turn wins
    tr = ans["tree-0"]
    assert tr[0]["A"][2] is None and tr[0]["A"][4] is True
    assert tr[1]["A"][2] == "B" and tr[1]["A"][4] is False and tr[1]["B"][3] == ["A"]
    assert tr[3]["A"][2] == "B" and tr[3]["A"][1][0][0] == "C"    # not first: the parent stays
    assert tr[6]["A"][2] == "C"
    n_ops = sum(len(a) for a in ans.values())
    assert n_ops >= 300


def _sequential_vs_closed(script):
    """Every update_batch (and update) of the script through the loop and through the closed form."""
    m, n, changed = K.Model(), 0, 0
    for op in script:
        if op[0] in ("update", "update_batch"):
            names = [op[1]] if op[0] == "update" else op[1]
            allow = ([op[2]] if op[0] == "update" else op[2]) if len(op) > 2 else None
            want_st = {}
            closed = K.batch_closed_form(m, names, allow)
            assert m.run(op, st=want_st) == closed, op
            n += 1
            changed += 1 if want_st.get("told_changed") else 0
        else:
            m.run(op)
    return n, changed


def test_closed_form_equals_the_loop_on_built_scripts():
    total = 0
    for name, script in K.built_scripts():
        total += _sequential_vs_closed(script)[0]
    for script in (K.script_batches(65, "shuffled"), K.script_batches(9, "asc", 1),
                   K.script_batches(5, "desc"), K.script_children(), K.script_observation_sets()):
        total += _sequential_vs_closed(script)[0]
    assert total > 200


def test_closed_form_equals_the_loop_on_seeded_scripts():
    reached = 0
    for seed in range(300):
        script = K.seeded_script(seed)
        st = {}
        K.run_script(script, stats=st)
        for k in ("slot_twice", "held_unobserved", "obs_not_holding", "obs_bad_kf"):
            assert st.get(k, 0) > 0, (seed, k)
        n, changed = _sequential_vs_closed(script)
        reached += 1 if changed else 0
    assert reached >= 50, reached


def test_shape_scripts_hit_their_sizes():
    a = K.run_script(K.script_observation_sets())
    assert [len(a[i]["QO%d_0" % n][0]) for i, n in enumerate((0, 1, 63, 64, 65, 200))] == [0, 1, 63, 64, 65, 200]
    assert len(a[6]["R"][0]) == 200 and len(a[6]["R"][1]) >= 1
    a = K.run_script(K.script_big_keyframe())
    g = a[0]["G"]
    assert dict(g[0]) == {"A": 14, "B": 15, "C": 4046, "D": 100, "E": 1}
    assert [o for o, _ in g[1]] == ["C", "D", "B"]
    a = K.run_script(K.script_children())
    assert [len(a[0][f"P{i}"][3]) for i in range(4)] == [1, 2, 65, 66] and a[2] == a[0] != a[1]
    s = K.script_many_neighbours(K.MAX_CONNECTIONS) + [("update", "Q")]
    a = K.run_script(s)
    assert len(a[0]["Q"][0]) == K.MAX_CONNECTIONS and a[0]["Q"][1] == [("W", 15)]
    for n in (1, 2, 5, 64, 65):
        a = K.run_script(K.script_batches(n, "shuffled"))
        assert len(a[0]) == n


def test_null_handles_without_a_device():
    """Every new entry point refuses a null handle before it touches a device."""
    L = native.lib()
    E = abi.ORBFE_ERR_ARG
    a = np.zeros(8, np.int32)
    u = np.ones(8, np.uint8)
    n, p, f = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    assert L.orbfe_map_update_connections(None, 8, abi.ptr(a), abi.ptr(u), abi.ptr(a), abi.ptr(a)) == E
    assert L.orbfe_map_update_connections(None, 0, None, None, None, None) == E
    assert L.orbfe_map_add_connection(None, 0, 1, 15) == E
    assert L.orbfe_map_erase_connection(None, 0, 1) == E
    assert L.orbfe_map_update_best_covisibles(None, 0) == E
    assert L.orbfe_map_erase_keyframe_connections(None, 0) == E
    assert L.orbfe_map_set_connections(None, 0, 8, abi.ptr(a), abi.ptr(a)) == E
    assert L.orbfe_map_set_ordered_connections(None, 0, 8, abi.ptr(a), abi.ptr(a)) == E
    assert L.orbfe_map_set_first_connection(None, 0, 1) == E
    assert L.orbfe_map_get_connections(None, 0, abi.ptr(a), abi.ptr(a), 8, C.byref(n)) == E
    assert L.orbfe_map_get_ordered_connections(None, 0, abi.ptr(a), abi.ptr(a), 8, C.byref(n)) == E
    assert L.orbfe_map_get_spanning_tree(None, 0, C.byref(p), C.byref(f), abi.ptr(a), 8, C.byref(n)) == E
    assert native.MAP_MAX_VOTED == K.MAX_CONNECTIONS
