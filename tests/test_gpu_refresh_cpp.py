"""Runs tests/cpp/refresh_test (built by __graft_entry__.build()) on the GPU: the C++ adapter's
MapPoint refresh (orbfe::LocalMap::RefreshPoints, UpdateNormalAndDepth,
ComputeDistinctiveDescriptors, RefreshKeyFramePoints, ProcessNewKeyFrame and the reference
keyframe through EraseObservation, include/orbfe_orbslam.hpp) on seeded maps, checked inside the
program after every step against MapPoint::UpdateNormalAndDepth / ComputeDistinctiveDescriptors /
EraseObservation and the loop of LocalMapping::ProcessNewKeyFrame written out over heap-allocated
stand-in structs with a real std::map<KF*, size_t> (order key = the pointer)."""
import os
import re
import subprocess

import pytest

BIN = os.path.join(os.path.dirname(__file__), "cpp", "build", "refresh_test")


@pytest.mark.gpu
def test_cpp_refresh():
    assert os.path.exists(BIN), "run __graft_entry__.build() first"
    moved = went = recent = 0
    for seed in (1, 2, 3, 4):
        r = subprocess.run([BIN, str(seed)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and f"refresh_test seed {seed}: ok" in r.stdout, r.stdout[-2000:] + r.stderr
        a, b, c = re.search(r"\((\d+) references moved, (\d+) points went bad, (\d+) recent\)", r.stdout).groups()
        moved, went, recent = moved + int(a), went + int(b), recent + int(c)
    assert moved >= 4 and went >= 1 and recent >= 4     # the paths were exercised
