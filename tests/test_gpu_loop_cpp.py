"""Runs tests/cpp/loop_test (built by __graft_entry__.build()) on the GPU: the three loop-closing
methods of orbfe::ORBmatcher (include/orbfe_orbslam.hpp) on dumped cases.  SearchByProjection
gets Scw = 1.7 [R|t] and normalises it itself; SearchBySim3 gets s12 = 1.3, R12 and t12 and
evaluates sR12, sR21 and t21 itself; both build their own masks (spAlreadyFound, vbAlreadyMatched)
from ids.  Return values and vpMatched / vpMatches12 must equal the restatements'."""
import os
import subprocess

import numpy as np
import pytest

import fuse_cases as FC
import loop_cases as L

pytestmark = pytest.mark.gpu
BIN = os.path.join(os.path.dirname(__file__), "cpp", "build", "loop_test")


def test_cpp_loop_matchers(tmp_path):
    assert os.path.exists(BIN), "run __graft_entry__.build() first"
    sbp = dict(L.sbp_case(0))
    scw = (sbp["tcw"].astype(np.float32) * np.float32(1.7)).astype(np.float32)
    sbp["tcw"] = FC.sim3_normalise(scw)
    s3 = L.sim3_case(0, mixed=True)
    assert abs(float(s3["s12"]) - 1.0) > 0.1
    bow = L.bow_case(0)
    path = str(tmp_path / "loop_case.bin")
    L.dump_case(path, sbp, scw, s3, bow)
    r = subprocess.run([BIN, path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "LOOP DONE" in r.stdout, r.stdout[-2000:] + r.stderr
    got = {}
    for line in r.stdout.splitlines():
        w = line.split()
        if len(w) == 2 and w[1].startswith("n="):
            got[w[0]] = [int(w[1][2:]), None]
        elif w and w[0].endswith("_OUT"):
            got[w[0][:-4]][1] = np.array([int(x) for x in w[1:]], np.int32)

    matched, n, _, bad = L.loop_sbp(sbp, sbp["th"])
    assert not bad and n >= 40
    assert got["SBP"][0] == n and np.array_equal(got["SBP"][1], matched)

    m12, _, _, nf, bad = L.sim3(s3)
    assert not bad and nf >= 40
    exp = s3["matches12"].copy()
    exp[m12 >= 0] = s3["pts2"]["ids"][m12[m12 >= 0]]
    assert got["SIM3"][0] == nf and np.array_equal(got["SIM3"][1], exp)

    b12, nb = L.bow_kk(bow, 0.75, True)
    exp = np.where(b12 >= 0, 1000 + b12, -1)
    assert nb >= 40 and got["BOW"][0] == nb and np.array_equal(got["BOW"][1], exp)
