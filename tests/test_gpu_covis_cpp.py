"""Runs tests/cpp/covis_test (built by __graft_entry__.build()) on the GPU: the C++ adapter's
covisibility graph (orbfe::LocalMap::UpdateConnections and its companions,
include/orbfe_orbslam.hpp) on seeded maps, checked inside the program against
KeyFrame::UpdateConnections / AddConnection / UpdateBestCovisibles / EraseConnection /
GetCovisiblesByWeight written out over heap-allocated stand-in structs with a real
std::map<KF*, int>, std::vector and std::list (order key = the pointer): the online sequence, the
load-map loop and GetCovisiblesByWeight at its quirk; and the program's --time mode, which needs
no device."""
import os
import subprocess

import pytest

BIN = os.path.join(os.path.dirname(__file__), "cpp", "build", "covis_test")


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_cpp_covisibility(seed):
    assert os.path.exists(BIN), "run __graft_entry__.build() first"
    r = subprocess.run([BIN, str(seed)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "COVIS DONE" in r.stdout, r.stdout[-2000:] + r.stderr
    done = dict(w.split("=") for w in r.stdout.splitlines()[-1].split()[2:])
    assert int(done["bad"]) == 0 and int(done["steps"]) > 50
    assert int(done["inversions"]) > 3      # address order is not id order: the keys matter
    assert int(done["quirk"]) > 0           # lists whose every weight is >= w: the reference returns nothing
    assert int(done["resorted"]) > 0        # lists that a changed AddConnection re-sorted in full


def test_cpp_time_mode_needs_no_device():
    assert os.path.exists(BIN), "run __graft_entry__.build() first"
    r = subprocess.run([BIN, "--time", "2"], capture_output=True, text=True, timeout=120)
    lines = r.stdout.splitlines()
    assert r.returncode == 0 and len(lines) == 2, r.stdout + r.stderr
    assert lines[0].startswith("TIME online keyframes=60") and lines[1].startswith("TIME loadmap keyframes=1000")
