"""Runs tests/cpp/rgbd_test (built by __graft_entry__.build()) on the GPU: the adapter's
ORBextractor::ComputeStereoFromRGBD (foreign pointer and depth buffer) and ORBmatcher::ClosePoints
(include/orbfe_orbslam.hpp) against the reference's lookup loop and its std::sort-and-walk written
out literally in the program, compared on float bits there."""
import os
import re
import subprocess

import pytest

pytestmark = pytest.mark.gpu
BIN = os.path.join(os.path.dirname(__file__), "cpp", "build", "rgbd_test")


def test_cpp_rgbd_path():
    assert os.path.exists(BIN), "run __graft_entry__.build() first"
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "RGBD DONE" in r.stdout and "MISMATCH" not in r.stdout, \
        r.stdout[-2000:] + r.stderr
    m = re.search(r"STEREO n=(\d+) with_depth=(\d+)", r.stdout)
    assert m and int(m.group(1)) == 400 and 300 <= int(m.group(2)) < 400
    visited = [int(v) for v in re.findall(r"CLOSE mode=\d th=\S+ visited=(\d+)", r.stdout)]
    n = int(m.group(2))
    # more than 100 inside th: the cut follows them; fewer: 101 visits; th beyond all, and
    # StereoInitialization: every feature with depth
    assert len(visited) == 4 and 101 < visited[0] < n and visited[1] == 101 and visited[2] == visited[3] == n
