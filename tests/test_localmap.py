"""The local map's restatement (tests/localmap_cases.py) is a fit yardstick: its built cases reach
every branch, every single-decision mutant changes an answer on them, and they are not trivial;
and the library refuses null handles and bad arguments without a device.  The comparison of the
library with the restatement is in tests/test_gpu_localmap.py."""
import ctypes as C
import inspect
import re

import numpy as np
import pytest

import localmap_cases as K
from orbslam_mapsave_amd import abi, native


@pytest.fixture(scope="module")
def baseline():
    stats = {}
    ans = {name: K.run_script(script, stats=stats) for name, script in K.built_scripts()}
    return ans, stats


def test_every_branch_is_reached(baseline):
    _, stats = baseline
    expected = {"frame_null", "frame_live", "frame_bad", "vote", "empty_return", "p1_bad",
                "p1_newmax", "p1_tie", "p1_below", "p1_all_bad", "limit_break", "neigh_absent",
                "neigh_bad", "neigh_stamped", "neigh_pushed", "neigh_none", "child_bad",
                "child_stamped", "child_pushed", "child_none", "parent_none", "parent_stamped",
                "parent_pushed", "parent_bad_pushed", "ref_set", "ref_kept", "pt_kf_bad",
                "pt_null", "pt_stamped", "pt_bad", "pt_pushed"}
    src = inspect.getsource(K.Model)
    emitted = set(re.findall(r'_bump\(st, "(\w+)"', src)) | {"parent_bad_pushed", "parent_pushed"}
    assert emitted == expected, emitted ^ expected
    assert set(stats) == expected, expected ^ set(stats)
    low = {k: v for k, v in stats.items() if v < 5}
    assert not low, low


def test_required_mutants_are_present():
    assert len(K.MUTANTS) == len(set(K.MUTANTS)) == 18
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
    v0 = ans["votes-0"]
    # keys run against the slots in variant 0: the list is in key order, K5 (bad, most votes) is
    # out, K3 and K1 tie at 2 and the lower key (K3) is the reference keyframe
    assert v0[0][0] == ["K3", "K1", "K0"] and v0[0][1] == "K3"
    assert v0[0][3][4] is None and v0[0][3][0] == "K1_0"          # the bad frame point is NULLed
    assert v0[1][0] == v0[0][0] and v0[1][2] == [] and v0[0][2]   # same frame id: no points left
    assert v0[2][0] == v0[1][0] and v0[2][2] == v0[0][2]          # empty vote: the old list again
    assert v0[3][0] == [] and v0[3][1] == v0[2][1]                # all bad: empty list, old reference
    n0 = ans["neighbours-0"]
    assert "K7" in n0[0][0] and "K8" not in n0[0][0] and "K9" not in n0[0][0] and "K10" not in n0[0][0]
    assert "K8" in n0[2][0]
    f0 = ans["family-0"]
    assert f0[0][0] == ["A", "B", "C", "NA", "E1", "NB", "PB"]     # E1 by key; C is never visited
    assert f0[0][4]["PB"] == 7 and "PB_0" in f0[0][2]              # the bad parent: stamped, its points listed
    assert f0[1][0] == ["A", "B", "C", "NA", "E1", "P2"]           # three pushes, then the break
    assert len(f0[1][0]) < len(f0[2][0])
    g = ans["gate-0"]
    assert [len(a[0]) for a in g] == [82, 81, 82, 81, 82]
    p0 = ans["points-0"]
    assert p0[0][2].count("ALL") == 1 and "BAD" not in p0[0][2] and "OLD" not in p0[0][2]
    assert p0[0][0][-1] == "K4" and "K4_0" in p0[0][2]
    n_updates = sum(len(a) for a in ans.values())
    assert n_updates >= 100 and sum(1 for a in ans.values() for u in a if u[2]) >= 70


def test_seeded_scripts_run():
    stats = {}
    out = K.run_script(K.seeded_script(1, 80), stats=stats)
    assert len(out) > 20 and stats.get("neigh_pushed", 0) > 0 and stats.get("pt_stamped", 0) > 0


def test_shape_scripts_hit_their_sizes():
    a = K.run_script(K.script_many_keyframes(K.MAX_VOTED))
    assert len(a[0][0]) == K.MAX_VOTED and len(a[0][2]) == K.MAX_VOTED
    a = K.run_script(K.script_point_lists(1024))
    assert [len(u[2]) for u in a[:7]] == [1023, 1024, 1025, 2047, 2048, 2049, 8192]
    a = K.run_script(K.script_children())
    assert len(a[0][0]) == 4 + 3 and a[1][0][:4] == a[0][0][:4]
    a = K.run_script(K.script_observation_sets())
    assert [len(u[0]) for u in a[:6]] == [0, 1, 63, 64, 65, 200]


def test_bad_arguments_without_a_device():
    """Every entry point refuses a null handle before it touches a device.  The refusals that
    need a live handle (out-of-range slots, a duplicate key, 8193 slots, 11 neighbours) are in
    tests/test_gpu_localmap.py: a handle cannot be created without a device."""
    L = native.lib()
    E = abi.ORBFE_ERR_ARG
    st = C.c_int(0)
    a = np.zeros(8, np.int32)
    u = np.zeros(8, np.uint64)
    n, r, s = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    p = C.c_void_p(0)
    arr = native.MapPointArrays()
    assert not L.orbfe_map_create(0, -1, 0, C.byref(st)) and st.value == E
    assert not L.orbfe_map_create(-1, 0, 0, C.byref(st)) and st.value in (E, abi.ORBFE_ERR_HIP)
    L.orbfe_map_destroy(None)
    assert L.orbfe_map_set_stream(None, None) == E
    assert L.orbfe_map_clear(None) == E
    assert L.orbfe_map_size(None, C.byref(n), C.byref(r)) == E
    assert L.orbfe_map_add_keyframe(None, 1, 8, abi.ptr(a), C.byref(s)) == E
    assert L.orbfe_map_set_keyframe_points(None, 0, 0, 8, abi.ptr(a)) == E
    assert L.orbfe_map_set_keyframe_bad(None, 0, 1) == E
    assert L.orbfe_map_set_covisibility(None, 0, 8, abi.ptr(a)) == E
    assert L.orbfe_map_set_children(None, 0, 8, abi.ptr(a)) == E
    assert L.orbfe_map_set_parent(None, 0, -1) == E
    assert L.orbfe_map_add_points(None, 8, C.byref(s)) == E
    assert L.orbfe_map_set_points_bad(None, 8, abi.ptr(a), 1) == E
    assert L.orbfe_map_add_observations(None, 8, abi.ptr(a), abi.ptr(a)) == E
    assert L.orbfe_map_erase_observations(None, 8, abi.ptr(a), abi.ptr(a)) == E
    assert L.orbfe_map_set_stamps(None, 0, 8, abi.ptr(a), abi.ptr(u)) == E
    assert L.orbfe_map_get_stamps(None, 1, 8, abi.ptr(a), abi.ptr(u)) == E
    assert L.orbfe_map_set_local_keyframes(None, 8, abi.ptr(a), -1) == E
    assert L.orbfe_map_get_local_keyframes(None, abi.ptr(a), 8, C.byref(n), C.byref(r)) == E
    assert L.orbfe_map_update_local(None, 1, 8, abi.ptr(a), abi.ptr(a), 8, C.byref(n), C.byref(r),
                                    abi.ptr(a), 8, C.byref(s)) == E
    assert L.orbfe_map_update_local_device(None, 1, 0, None, abi.ptr(a), 8, C.byref(n), C.byref(r),
                                           C.byref(s)) == E
    assert L.orbfe_map_local_points_device(None, C.byref(p), C.byref(n)) == E
    assert L.orbfe_map_get_local_points(None, abi.ptr(a), 8, C.byref(n)) == E
    assert L.orbfe_map_gather_points_device(None, 0, None, C.byref(arr), C.byref(arr)) == E
    assert C.sizeof(native.MapPointArrays) == 72
    assert native.MAP_MAX_VOTED == K.MAX_VOTED and native.MAP_MAX_KF_SLOTS == K.MAX_KF_SLOTS
