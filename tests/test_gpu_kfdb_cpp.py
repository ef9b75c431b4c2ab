"""Runs tests/cpp/kfdb_test (built by __graft_entry__.build()) on the GPU: the C++ adapter's
ORBVocabulary::score and KeyFrameDatabase (include/orbfe_orbslam.hpp) on seeded scripts of adds,
erases, covisibility lists and queries, checked inside the program against its own std::list
inverted file; and the program's --time mode, which needs no device."""
import os
import subprocess

import pytest

import kfdb_cases as K
from orbslam_mapsave_amd.synth import synthetic_vocabulary_text

BIN = os.path.join(os.path.dirname(__file__), "cpp", "build", "kfdb_test")


@pytest.mark.gpu
@pytest.mark.parametrize("scoring", [0, 1, 2, 4, 5])
def test_cpp_keyframe_database(scoring, tmp_path):
    assert os.path.exists(BIN), "run __graft_entry__.build() first"
    voc = str(tmp_path / "voc.txt")
    synthetic_vocabulary_text(voc, 5, 4, seed=2, scoring=scoring, weighting=0)  # 625 words
    script = K.seeded_script(50 + scoring, 160, nkf0=30)
    want = K.run_script(script, scoring)
    path = str(tmp_path / "script.bin")
    K.dump_script(path, scoring, script)
    r = subprocess.run([BIN, voc, path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "KFDB DONE" in r.stdout, r.stdout[-2000:] + r.stderr
    done = dict(w.split("=") for w in r.stdout.splitlines()[-1].split()[2:])
    assert int(done["bad"]) == 0 and int(done["queries"]) == len(want) > 20
    assert int(done["nonempty"]) == sum(1 for a in want if a[0]) > 10 and int(done["scores"]) > 30
    # the program's own restatement agrees with the Python one on every query
    q = [l.split() for l in r.stdout.splitlines() if l.startswith("Q ")]
    assert [int(w[3].split("=")[1]) for w in q] == [len(a[0]) for a in want]
    assert [w[4] == "h18=1" for w in q] == [a[1] for a in want]


def test_cpp_time_mode_needs_no_device(tmp_path):
    assert os.path.exists(BIN), "run __graft_entry__.build() first"
    path = str(tmp_path / "script.bin")
    K.dump_script(path, 0, K.seeded_script(3, 60, nkf0=40))
    r = subprocess.run([BIN, "--time", path, "2"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("TIME keyframes="), r.stdout + r.stderr
