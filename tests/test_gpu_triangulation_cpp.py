"""Runs tests/cpp/triangulation_test (built by __graft_entry__.build()) on the GPU:
orbfe::ORBmatcher::SearchForTriangulation of include/orbfe_orbslam.hpp on a dumped case whose
epipole is not rounded, so the adapter's evaluation of ORBmatcher.cc:667-673 from the pose must
give the float the restatement was handed.  nmatches and the pair list must be identical, with the
adapter's default (the reference as written, no blocking) and with blockMatched2."""
import os
import subprocess

import numpy as np
import pytest

import triangulation_cases as TC

pytestmark = pytest.mark.gpu
BIN = os.path.join(os.path.dirname(__file__), "cpp", "build", "triangulation_test")


@pytest.mark.parametrize("check_ori,only_stereo", [(False, False), (True, False), (True, True)])
def test_cpp_search_for_triangulation(tmp_path, check_ori, only_stereo):
    assert os.path.exists(BIN), "run __graft_entry__.build() first"
    c = TC.tri_case(3, 0.7, round_epipole=False)
    ex, ey = TC.epipole_of(*c["pose"])
    assert c["epipole"][0] == ex and c["epipole"][1] == ey and float(ex) * 4 != round(float(ex) * 4)
    path = str(tmp_path / "tri_case.bin")
    TC.dump_case(path, c, check_ori, only_stereo)
    r = subprocess.run([BIN, path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "TRIANGULATION DONE" in r.stdout, r.stdout[-2000:] + r.stderr
    got = {}
    for line in r.stdout.splitlines():
        w = line.split()
        if w[0] == "BLOCK":
            cur = got[int(w[1])] = dict(n=int(w[2].split("=")[1]), pairs=[])
        elif w[0] == "P":
            cur["pairs"].append((int(w[1]), int(w[2])))
    for block in (0, 1):
        _, n, pairs = TC.restated(c, check_ori, bool(block), only_stereo)
        assert n > 40 and got[block]["n"] == n
        assert got[block]["pairs"] == [tuple(p) for p in pairs.tolist()]
    assert got[0]["pairs"] != got[1]["pairs"]
