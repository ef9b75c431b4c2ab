"""Runs tests/cpp/culling_test (built by __graft_entry__.build()) on the GPU: the C++ adapter's
culling (orbfe::LocalMap::MapPointCulling, KeyFrameCulling, SetKeyFrameBadFlag, SetErase and the
observation calls with indices, include/orbfe_orbslam.hpp) on seeded dense maps, checked inside
the program after every step against LocalMapping::MapPointCulling / KeyFrameCulling,
MapPoint::AddObservation / EraseObservation / SetBadFlag and KeyFrame::SetBadFlag / SetErase written
out over heap-allocated stand-in structs with a real std::map<KF*, size_t>, std::set<KF*> and
std::list<MP*> (order key = the pointer); and the program's --time mode, which needs no device."""
import os
import re
import subprocess

import pytest

BIN = os.path.join(os.path.dirname(__file__), "cpp", "build", "culling_test")


@pytest.mark.gpu
def test_cpp_culling():
    assert os.path.exists(BIN), "run __graft_entry__.build() first"
    multi = 0
    for seed in (1, 2, 3, 4, 5, 6):
        r = subprocess.run([BIN, str(seed)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and f"culling_test seed {seed}: ok" in r.stdout, r.stdout[-2000:] + r.stderr
        multi += int(re.search(r"\((\d+) calls culled two or more", r.stdout).group(1))
    assert multi >= 2     # the sequential dependence was exercised


def test_cpp_time_mode_needs_no_device():
    assert os.path.exists(BIN), "run __graft_entry__.build() first"
    r = subprocess.run([BIN, "--time", "1"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "literal KeyFrameCulling, 30 x 1000" in r.stdout and "literal MapPointCulling, 500 points" in r.stdout
