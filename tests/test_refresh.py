"""tests/refresh_cases.py is not trivial: every mutant changes an answer on a built case, every
branch is taken, the float sum's bits differ between key order and slot order and a median tie
falls between keys that run opposite to their slots on the restatement alone, refusals change
nothing; and every new entry point refuses a null handle and bad arguments before it touches a
device.  No GPU."""
import ctypes as C

import numpy as np

import refresh_cases as R
from orbslam_mapsave_amd import abi, native


def test_every_mutant_changes_an_answer():
    scripts = list(R.built_scripts())
    base = {name: R.run_script(s) for name, s in scripts}
    for mu in R.MUTANTS:
        killed = [name for name, s in scripts if R.run_script(s, mu) != base[name]]
        assert killed, mu


def test_every_branch_is_taken():
    st = {}
    for _, s in R.built_scripts():
        R.run_script(s, stats=st)
    for k in ("dd_all_bad", "dd_bad", "dd_bad_observer", "dd_empty", "dd_tie", "dd_written",
              "erase_ref_bad", "erase_ref_empty", "erase_ref_key_not_slot", "erase_ref_next",
              "erase_ref_other", "list_null", "list_repeat", "nd_bad", "nd_bad_observer", "nd_empty",
              "nd_null_ref", "nd_ref_absent", "nd_ref_bad", "nd_ref_observer", "nd_unsupported",
              "nd_written", "pk_bad", "pk_null", "pk_observed", "pk_second_index", "add_right",
              "add_left_only", "erase_to_bad", "kfbad_point_bad", "kfbad_second_index"):
        assert st.get(k, 0) >= 5, (k, st.get(k, 0))


def test_the_sum_depends_on_the_order():
    """On the restatement alone: the same terms added in slot order give other bits, and the keys
    of that case run opposite to the slots."""
    for v in range(5):
        s = R.case_sum_order(v)
        m = R.Model()
        for op in s:
            if op[0] == "refresh":
                break
            m.run(op)
        keys = [m.kfs[f"K{i}"].key for i in range(len(m.kfs))]
        assert keys == sorted(keys, reverse=True)
        a, b = R.Model(), R.Model()
        for op in s:
            a.run(op)
            b.run(op, "sum_slot_order")
        assert a.mps["P0"].normal.tobytes() != b.mps["P0"].normal.tobytes()
        # the terms themselves: ones and values near 2^-24
        x = sorted(abs(float(m.mps["P0"].pos[0] - kf.center[0])) for kf in m.kfs.values())
        assert x[0] < 2.0 ** -20 and x[-1] >= 1.0


def test_the_median_tie_is_between_reversed_keys():
    for v in range(5):
        s = R.case_median_tie(v)
        st = {}
        base = R.run_script(s, stats=st)
        assert st["dd_tie"] >= 2
        assert R.run_script(s, "tie_slot_order") != base and R.run_script(s, "tie_last") != base
        m = R.Model()
        for op in s:
            m.run(op)
        assert m.kfs["K0"].key > m.kfs["K1"].key > m.kfs["K2"].key


def test_refusals_change_nothing():
    n = 0
    for _, s in R.built_scripts():
        m, prev = R.Model(), None
        for op in s:
            a = m.run(op)
            if a is not None and a[0] in ("error", "capacity"):
                assert prev is not None and a[1] == prev
                n += 1
            prev = m.state()
    assert n >= 10


def test_observer_count_scripts_reach_their_sizes():
    for n in (0, 1, 2, 3, 4, 5, 63, 64, 65, 200):
        for v in (0, 1, 2):
            m = R.Model()
            for op in R.script_observer_count(n, v):
                a = m.run(op)
            assert len(m.mps["P"].obs) == n
            assert a[0] == [R.ND | R.DESC if n else 0, 0]
    m = R.Model()
    for op in R.script_observer_count(1025):
        a = m.run(op)
    assert a[0] == "capacity"


def test_null_handles_and_bad_arguments_are_refused_without_a_device():
    L = native.lib()
    f3 = (C.c_float * 3)()
    i1 = (C.c_int32 * 1)()
    n = C.c_int32(0)
    arr = native.MapPointArrays()
    E = abi.ORBFE_ERR_ARG
    assert L.orbfe_map_set_scale_factors(None, 3, f3) == E
    assert L.orbfe_map_get_scale_factors(None, f3, 3, C.byref(n)) == E
    assert L.orbfe_map_set_keyframe_centers(None, 1, i1, f3) == E
    assert L.orbfe_map_get_keyframe_centers(None, 1, i1, f3) == E
    assert L.orbfe_map_set_keyframe_descriptors(None, 0, 0, None) == E
    assert L.orbfe_map_set_keyframe_descriptors_device(None, 0, 0, None) == E
    assert L.orbfe_map_get_keyframe_descriptors(None, 0, 0, None, C.byref(n), None) == E
    assert L.orbfe_map_set_point_ref_keyframes(None, 1, i1, i1) == E
    assert L.orbfe_map_get_point_ref_keyframes(None, 1, i1, i1) == E
    assert L.orbfe_map_refresh_points(None, 3, 1, i1, C.byref(arr), None) == E
    assert L.orbfe_map_refresh_points_device(None, 3, 1, i1, C.byref(arr), None) == E
    assert L.orbfe_map_refresh_keyframe_points(None, 0, 3, C.byref(arr), C.byref(n)) == E
    assert L.orbfe_map_process_new_keyframe(None, 0, C.byref(arr), i1, 1, C.byref(n)) == E


def test_helpers_are_the_stated_float_operations():
    """recip, axpy and mean against the same operations spelled out with explicit roundings."""
    rng = np.random.default_rng(3)
    for _ in range(200):
        d, acc = np.float32(rng.normal()), np.float32(rng.normal())
        s = float(abs(rng.normal())) + 0.1
        a = R.recip(s)
        assert a.dtype == np.float32 and a == np.float32(1.0 / s)
        assert R.axpy(acc, d, a) == np.float32(np.float32(d * a) + acc)
        n = int(rng.integers(1, 40))
        assert R.mean(acc, n) == np.float32(acc * np.float32(1.0 / n))
