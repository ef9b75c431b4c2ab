"""Runs tests/cpp/fuse_test (built by __graft_entry__.build()) on the GPU: both
orbfe::ORBmatcher::Fuse overloads of include/orbfe_orbslam.hpp on a dumped case, with recording
callables.  nFused, the call sequence (on_occupied / on_empty, list entry, keypoint) and the final
slots must equal the Python walk over the restatement's search; the Sim3 overload gets
Scw = 1.7 [R|t] and normalises it itself."""
import os
import subprocess

import numpy as np
import pytest

import fuse_cases as FC

pytestmark = pytest.mark.gpu
BIN = os.path.join(os.path.dirname(__file__), "cpp", "build", "fuse_test")
TH = {FC.SE3: 3.0, FC.SIM3: 4.0}


def test_cpp_fuse_walk(tmp_path):
    assert os.path.exists(BIN), "run __graft_entry__.build() first"
    c, pid = FC.walk_case(0)
    scw = (c["tcw"].astype(np.float32) * np.float32(1.7)).astype(np.float32)
    path = str(tmp_path / "fuse_case.bin")
    FC.dump_case(path, c, FC.MapModel(c["kf"].n, pid, 0), TH[FC.SE3], TH[FC.SIM3], scw)
    r = subprocess.run([BIN, path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "FUSE DONE" in r.stdout, r.stdout[-2000:] + r.stderr
    got = {}
    for line in r.stdout.splitlines():
        w = line.split()
        if w[0] == "MODE":
            cur = got[w[1]] = dict(n=int(w[2].split("=")[1]), calls=[], slots=None)
        elif w[0] in ("O", "E"):
            cur["calls"].append((w[0], int(w[1]), int(w[2])))
        elif w[0] == "SLOTS":
            cur["slots"] = [int(x) for x in w[1:]]
    for name, mode in (("SE3", FC.SE3), ("SIM3", FC.SIM3)):
        model = FC.MapModel(c["kf"].n, pid, 0)
        cm = dict(c, skip=model.static_skip())
        if mode == FC.SIM3:
            cm["tcw"] = FC.sim3_normalise(scw)
        bi, _, _, bad = FC.restated(cm, TH[mode], mode)
        assert not bad
        n = FC.walk(model, bi, mode)
        assert n > 30 and got[name]["n"] == n
        assert got[name]["calls"] == model.calls
        assert got[name]["slots"] == model.slot.tolist()
        assert {k for k, _, _ in model.calls} == {"O", "E"}
