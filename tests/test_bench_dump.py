"""bench.py's plain run and --dump-outputs: the result line of a plain run (the timed steps only,
--steps of them, ms_per_step, none of the --full legs), and the dumped arrays — float .npy files
holding what the last timed step left in the output buffers, rows past a frame's keypoint count
zeroed, equal to the oracle's extraction and brute-force match of the same seeded frames."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench
from orbslam_mapsave_amd.abi import KEYPOINT_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _as_float(kps):
    return np.stack([kps[f].astype(np.float32) for f in KEYPOINT_DTYPE.names], -1)


def test_extract_outputs_layout():
    """extract_outputs on host tensors: every frame's count, a fixed sample of the frames, the
    seven keypoint fields as float32, and zeros past each frame's count whatever the buffers
    hold there."""
    import torch
    B, cap = 2 * bench.DUMP_FRAMES + 3, 5
    rng = np.random.default_rng(1)
    kps = np.zeros((B, cap), KEYPOINT_DTYPE)
    for f in ("x", "y", "size", "angle", "response"):
        kps[f] = rng.uniform(1, 100, (B, cap)).astype(np.float32)
    kps["octave"] = rng.integers(0, 8, (B, cap))
    kps["class_id"] = -1
    desc = rng.integers(1, 256, (B, cap, 32), dtype=np.uint8)
    out = rng.integers(1, 256, (B, cap, 3)).astype(np.int32)
    n = rng.integers(0, cap + 1, B).astype(np.int32)
    args = (torch.from_numpy(kps.view(np.uint8).reshape(B, cap * 28)), torch.from_numpy(desc),
            torch.from_numpy(n), torch.from_numpy(out), cap)
    got = bench.extract_outputs(*args)
    again = bench.extract_outputs(*args)
    assert set(got) == {"counts", "frame_index", "keypoints", "descriptors", "matches"}
    assert all(a.dtype == np.float32 for a in got.values())
    assert all(np.array_equal(got[k], again[k]) for k in got)  # the same sample every time
    sel = got["frame_index"].astype(np.int64)
    assert len(sel) == bench.DUMP_FRAMES == len(set(sel)) and np.all(np.diff(sel) > 0)
    assert np.array_equal(got["counts"], n.astype(np.float32))
    live = np.arange(cap)[None, :] < n[sel][:, None]
    assert np.array_equal(got["keypoints"], _as_float(kps[sel]) * live[:, :, None])
    assert np.array_equal(got["descriptors"], desc[sel].astype(np.float32) * live[:, :, None])
    assert np.array_equal(got["matches"], out[sel].astype(np.float32) * live[:, :, None])
    # extract only (config 2): no match rows
    assert "matches" not in bench.extract_outputs(args[0], args[1], args[2], None, cap)


@pytest.mark.gpu
def test_plain_run_dumps_what_it_computed(tmp_path):
    import oracle
    from orbslam_mapsave_amd.synth import synthetic_batch, synthetic_frame
    B = 6
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2",
           "--warmup", "1", "--batch", str(B), "--distinct", str(B), "--settle-s", "0",
           "--dump-outputs", str(tmp_path / "dump")]  # the default reading, x86: the oracle's too
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    line = json.loads(lines[0])
    assert line["metric"] == bench.METRIC and line["unit"] == "frames/s"
    assert line["higher_is_better"] is True and line["dtype"] == "u8"
    assert line["steps"] == 2 and line["warmup"] == 1 and line["full"] is False
    assert line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(B / (line["ms_per_step"] / 1e3), rel=0.02)
    for leg in ("roofline", "cpu_baseline", "stage_ms_per_step", "soak"):
        assert leg not in line

    files = sorted(os.listdir(tmp_path / "dump"))
    assert files == ["counts.npy", "descriptors.npy", "frame_index.npy", "keypoints.npy",
                     "matches.npy"]
    got = {f[:-4]: np.load(tmp_path / "dump" / f) for f in files}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64 << 20
    assert np.array_equal(got["frame_index"], np.arange(B))  # fewer frames than the sample: all

    frames = synthetic_batch(B, 640, 480, first_seed=0, distinct=B)
    p1 = oracle.params(1000, *bench.ORB)
    with oracle.variant(oracle.VAR_X86):
        ref = oracle.extract(oracle.params(2000, *bench.ORB), synthetic_frame(999_999, 640, 480))[1]
        mine = [oracle.extract(p1, frames[f]) for f in range(B)]
    for f in range(B):
        kps, desc = mine[f]
        n = len(kps)
        assert got["counts"][f] == n > 0
        assert np.array_equal(got["keypoints"][f, :n], _as_float(kps))
        assert np.array_equal(got["descriptors"][f, :n], desc.astype(np.float32))
        bi, bd, sd = oracle.bf_match(desc, ref)
        assert np.array_equal(got["matches"][f, :n], np.stack([bi, bd, sd], 1).astype(np.float32))
        for k in ("keypoints", "descriptors", "matches"):
            assert not got[k][f, n:].any()
