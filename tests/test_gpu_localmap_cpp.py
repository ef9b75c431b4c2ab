"""Runs tests/cpp/localmap_test (built by __graft_entry__.build()) on the GPU: the C++ adapter's
LocalMap (include/orbfe_orbslam.hpp) on seeded maps and walks of mutations and updates, checked
inside the program against Tracking::UpdateLocalKeyFrames / UpdateLocalPoints written out over
heap-allocated stand-in structs with a real std::map<KF*, int> and std::set<KF*> (order key = the
pointer); and the program's --time mode, which needs no device."""
import os
import subprocess

import pytest

BIN = os.path.join(os.path.dirname(__file__), "cpp", "build", "localmap_test")


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_cpp_local_map(seed):
    assert os.path.exists(BIN), "run __graft_entry__.build() first"
    r = subprocess.run([BIN, str(seed), "40"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "LOCALMAP DONE" in r.stdout, r.stdout[-2000:] + r.stderr
    done = dict(w.split("=") for w in r.stdout.splitlines()[-1].split()[2:])
    assert int(done["bad"]) == 0 and int(done["updates"]) == 40 and int(done["nonempty"]) > 20
    assert int(done["inversions"]) > 10      # address order is not id order: the keys matter


def test_cpp_time_mode_needs_no_device():
    assert os.path.exists(BIN), "run __graft_entry__.build() first"
    r = subprocess.run([BIN, "--time", "2"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("TIME keyframes="), r.stdout + r.stderr
