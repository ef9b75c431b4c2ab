#!/usr/bin/env python3
"""Times the MapPoint refresh of one keyframe on the device against the only route the map had
before it: one 1,000-point keyframe, every point with 5-30 observers.

    refresh_keyframe_points, both bits        2 launches, 1 host wait
    refresh_keyframe_points, descriptor bit   2 launches, 1 host wait
    read the rows back, gather on the host, orbfe_distinctive_descriptors (host form)
                                              1 row read-back per point (2 waits each), 1 launch

Host clock around calls that end in a wait on the device; the median of `--reps` calls after
three warm-ups, with the 10th and 90th percentiles.  Prints one JSON line per route and appends them to $BENCH_OUT/refresh_rows.jsonl
when BENCH_OUT is set.  Needs a GPU."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1000)
    ap.add_argument("--keyframes", type=int, default=30)
    ap.add_argument("--reps", type=int, default=500)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    torch.zeros(1, device="cuda:0")
    from orbslam_mapsave_amd import native

    rng = np.random.default_rng(11)
    P, K = a.points, a.keyframes
    lm = native.LocalMap(0, K, P)
    lm.add_points(P)
    lm.SetScaleFactors([1.2 ** i for i in range(8)])
    descs = rng.integers(0, 256, (K, P, 32), dtype=np.uint8)
    keys = np.array([0x7F0000000000 + 64 * (int(rng.integers(0, K)) * K + k) for k in range(K)])   # distinct
    for k in range(K):
        lm.add_keyframe(int(keys[k]), P, list(range(P)))
        lm.set_keyframe_features(k, rng.integers(0, 8, P), None, None, 40.0)
        lm.SetDescriptors(k, descs[k])
    lm.SetCameraCenter(list(range(K)), rng.uniform(-3, 3, (K, 3)))
    mp, kf = [], []
    for p in range(P):
        obs = set(int(x) for x in rng.choice(K, int(rng.integers(5, 31)), replace=False)) | {0}
        mp += [p] * len(obs)
        kf += sorted(obs)
    lm.AddObservation(mp, kf, mp)
    lm.SetReferenceKeyFrame(list(range(P)), [0] * P)
    t = {"xyz": torch.from_numpy(rng.uniform(-8, 8, (P, 3)).astype(np.float32)).cuda(),
         "normal": torch.zeros(P, 3, device="cuda"), "min_dist": torch.zeros(P, device="cuda"),
         "max_dist": torch.zeros(P, device="cuda"), "desc": torch.zeros(P, 32, dtype=torch.uint8, device="cuda")}
    torch.cuda.synchronize()
    arr = native.MapPointArrays(**{k: v.data_ptr() for k, v in t.items()})
    matcher = native.ORBmatcher(device=0)

    def both():
        assert lm.RefreshKeyFramePoints(0, arr, 3) == P

    def desc_only():
        assert lm.RefreshKeyFramePoints(0, arr, 2) == P

    def host_route():
        off, rows = [0], []
        for p in lm.get_keyframe_points(0):
            ks, xs = lm.GetObservations(int(p))
            o = np.argsort(keys[ks])                  # pointer order decides the median tie
            rows.append(descs[ks[o], xs[o]])
            off.append(off[-1] + len(ks))
        return matcher.ComputeDistinctiveDescriptors(np.asarray(off, np.int32), np.concatenate(rows))

    def timed(fn, reps):
        for _ in range(3):
            fn()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
        return [float(x) for x in np.percentile(ts, [50, 10, 90])] + [float(min(ts))]

    desc_only()
    dev = t["desc"].cpu().numpy().copy()
    best, out = host_route()
    assert np.array_equal(dev, out), "the two routes disagree"
    rows = []
    for name, fn, reps, launches, waits in (
            ("refresh_keyframe_points, both bits", both, a.reps, 2, 1),
            ("refresh_keyframe_points, descriptor bit", desc_only, a.reps, 2, 1),
            ("row read-back + host gather + orbfe_distinctive_descriptors", host_route, max(a.reps // 25, 3),
             1, 2 * P + 2)):
        med, p10, p90, lo = timed(fn, reps)
        rows.append({"route": name, "points": P, "keyframes": K, "observations": len(mp),
                     "median_ms": round(med * 1e3, 4), "p10_ms": round(p10 * 1e3, 4), "p90_ms": round(p90 * 1e3, 4),
                     "min_ms": round(lo * 1e3, 4), "reps": reps,
                     "launches": launches, "host_waits": waits, "clock": "host, around a synchronous call"})
        print(json.dumps(rows[-1]), flush=True)
    if os.environ.get("BENCH_OUT"):
        os.makedirs(os.environ["BENCH_OUT"], exist_ok=True)
        with open(os.path.join(os.environ["BENCH_OUT"], "refresh_rows.jsonl"), "a") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
