#!/usr/bin/env python3
"""Throughput of the §8(f) rows on one MI355X next to their CPU oracle (one JSON line per row).

Each row: GPU path through the C ABI with inputs resident in HBM where the ABI has a device
form (colour extraction, stereo, BoW transform, distinctive descriptors), host forms otherwise
(relocalisation SearchByProjection, SearchByBoW: one keyframe / frame per call, as Tracking
calls them); K timed iterations after warm-up, torch.cuda.synchronize on both sides; the CPU
oracle (single thread, a port of the reference path) on the same inputs.  Algorithmic bytes per
unit are stated per row; the achieved GB/s is those bytes over the measured time.

Run on the GPU box: python tools/bench_rows.py > gpurun_out/rows.jsonl
"""
from __future__ import annotations

import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

torch.cuda.init()
DEV = torch.device("cuda", 0)
torch.zeros(1, device=DEV)

import oracle  # noqa: E402  (test infrastructure: the CPU-baseline legs)
from orbslam_mapsave_amd import native  # noqa: E402
from orbslam_mapsave_amd.synth import (synthetic_color_frame, synthetic_frame,  # noqa: E402
                                       synthetic_stereo_pair, synthetic_vocabulary_text)

HBM = 8000.0


def timed(fn, k, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(k):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / k


def cpu_timed(fn, budget=4.0):
    n, t0 = 0, time.perf_counter()
    while True:
        fn()
        n += 1
        el = time.perf_counter() - t0
        if el >= budget and n >= 2:
            return el / n


def emit(row, unit, units_per_call, t_gpu, t_cpu, nbytes, note, cpu_units=None):
    """t_gpu: seconds per GPU call of units_per_call units; t_cpu: seconds per CPU call of
    cpu_units units (default: the same)."""
    cu = units_per_call if cpu_units is None else cpu_units
    line = {"row": row, "unit": unit, "value": round(units_per_call / t_gpu, 2),
            "ms_per_call": round(t_gpu * 1e3, 4), "units_per_call": units_per_call,
            "achieved_GBs": round(nbytes / t_gpu / 1e9, 2),
            "hbm_frac": round(nbytes / t_gpu / 1e9 / HBM, 5),
            "bytes_per_call": int(nbytes),
            "cpu_value": round(cu / t_cpu, 3), "cpu_cores": 1, "cpu_kind": "port",
            "gpu_over_cpu": round((units_per_call / t_gpu) / (cu / t_cpu), 1), "note": note}
    print(json.dumps(line), flush=True)


def row_color():
    B, W, H = 256, 640, 480
    cf = np.stack([synthetic_color_frame(s % 16, W, H, 3) for s in range(B)])
    d_img = torch.from_numpy(cf).to(DEV)
    ex = native.ORBextractor(1000, 1.2, 8, 32, 7, device=0, max_width=W, max_height=H, max_batch=B)
    ex.set_stream(torch.cuda.current_stream(DEV).cuda_stream)
    cap = ex.capacity(W, H)
    k = torch.empty((B, cap * 28), dtype=torch.uint8, device=DEV)
    d = torch.empty((B, cap, 32), dtype=torch.uint8, device=DEV)
    n = torch.empty(B, dtype=torch.int32, device=DEV)
    rects = torch.from_numpy(np.tile(np.array([[200, 100, 400, 300]], np.int32), (B, 1))).to(DEV)

    def go():
        ex.extract_color_batch_device(d_img.data_ptr(), native.PIX_RGB, B, W, H, 3 * W, 3 * W * H,
                                      k.data_ptr(), cap, d.data_ptr(), n.data_ptr(),
                                      d_rects=rects.data_ptr())
    t = timed(go, 10)
    p = oracle.params(1000, 1.2, 8, 32, 7)
    m = np.ones((H, W), np.uint8)
    m[100:300, 200:400] = 0
    tc = cpu_timed(lambda: oracle.extract(p, oracle.cvt_gray(cf[0], native.PIX_RGB), m))
    emit("(f)1 colour + human-mask extraction (RGB 640x480, 1000 kp)", "frames/s", B, t, tc,
         B * (3 * W * H + W * H), "device batch of 256 RGB frames, rectangle mask; bytes = the "
         "level-0 kernel's RGB read + gray write (the rest is the c3 pipeline)", cpu_units=1)
    ex.close()


def row_single():
    """Tracking's per-frame call: ORBextractor::operator() on one 640x480 frame through the host
    ABI (upload, the whole pipeline, download of keypoints and descriptors), as Frame::ExtractORB
    issues it (Frame.cc:358-364) — the latency a drop-in replacement adds per tracked frame."""
    img = synthetic_frame(3, 640, 480)
    ex = native.ORBextractor(1000, 1.2, 8, 20, 7, device=0, max_width=640, max_height=480)
    t = timed(lambda: ex(img), 200)
    p = oracle.params(1000, 1.2, 8, 20, 7)
    tc = cpu_timed(lambda: oracle.extract(p, img))
    emit("single-frame ORBextractor::operator() latency (640x480, 1000 kp, host ABI)",
         "frames/s", 1, t, tc, 640 * 480 + 1000 * 60,
         "host ABI: one frame per call, H2D upload + pipeline + D2H, synchronous", cpu_units=1)
    # the zero-copy form (orbfe_input_buffer / orbfe_extract_staged): the caller's cvtColor
    # writes the gray frame into the handle's pinned staging buffer (written here once, outside
    # the timed calls: that write is the caller's own cvtColor output, not the extractor's work),
    # the GPU reads it in place and the outputs stay in the pinned output buffers
    buf = ex.input_buffer(640, 480)
    buf[:] = img
    k0, d0 = ex(img)
    ks, ds = ex.extract_staged(640, 480, copy_out=False)
    assert ks.tobytes() == k0.tobytes() and np.array_equal(ds, d0)
    t2 = timed(lambda: ex.extract_staged(640, 480, copy_out=False), 400)
    emit("single-frame ORBextractor::operator() latency, zero-copy staging (640x480, 1000 kp)",
         "frames/s", 1, t2, tc, 640 * 480 + 1000 * 60,
         "host ABI orbfe_extract_staged: frame in the handle's pinned buffer (the caller's cvtColor "
         "target), outputs left in pinned memory (orbfe_staged_outputs), one graph launch + one "
         "synchronisation per call", cpu_units=1)
    ex.close()
    # the same calls from C++ (the adapter program, as Frame::ExtractORB would make them): no
    # Python / ctypes in the loop
    import re
    import subprocess
    exe = os.path.join(ROOT, "tests", "cpp", "build", "adapter_test")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    m = re.search(r"LATENCY host_us=([0-9.]+) staged_copy_us=([0-9.]+) staged_us=([0-9.]+)", r.stdout)
    if r.returncode == 0 and m:
        for us, what in ((float(m.group(1)), "host form (orbfe::ORBextractor::operator(), frame copied in)"),
                         (float(m.group(3)), "zero-copy staging (orbfe_extract_staged, outputs in place)")):
            emit(f"single-frame latency from C++, {what} (640x480, 1000 kp)", "frames/s", 1, us * 1e-6, tc,
                 640 * 480 + 1000 * 60, "tests/cpp/adapter_test: mean of 2,000 calls after 100 warm-up "
                 "calls, C++ caller through include/orbfe_orbslam.hpp", cpu_units=1)
    # SearchByBoW(KeyFrame*, Frame&) from C++ (Tracking.cc:1014's per-frame call), GPU against the
    # one-thread CPU port in the same program
    mb = re.search(r"BOW_LATENCY gpu_us=([0-9.]+) cpu_us=([0-9.]+) nodes=(\d+)/(\d+)", r.stdout)
    if r.returncode == 0 and mb:
        gu, cu = float(mb.group(1)), float(mb.group(2))
        emit(f"(f)4 SearchByBoW from C++ (1000 x 1000 features, {mb.group(3)}/{mb.group(4)} nodes)",
             "calls/s", 1, gu * 1e-6, cu * 1e-6, 2000 * (32 + 8),
             "tests/cpp/adapter_test: orbfe::ORBmatcher::SearchByBoW vs oracle_search_by_bow, mean of "
             "2,000 calls after 100 warm-up calls each; one kernel launch per call, the orientation "
             "filter on the host", cpu_units=1)


def row_stereo():
    B, W, H = 128, 640, 480
    pairs = [synthetic_stereo_pair(s % 16, W, H) for s in range(B)]
    L = torch.from_numpy(np.stack([a for a, _ in pairs])).to(DEV)
    R = torch.from_numpy(np.stack([b for _, b in pairs])).to(DEV)
    el = native.ORBextractor(1000, 1.2, 8, 20, 7, device=0, max_width=W, max_height=H, max_batch=B)
    er = native.ORBextractor(1000, 1.2, 8, 20, 7, device=0, max_width=W, max_height=H, max_batch=B)
    s = torch.cuda.current_stream(DEV).cuda_stream
    el.set_stream(s)
    er.set_stream(s)
    cap = el.capacity(W, H)
    bufs = {}
    for side, e, X in (("l", el, L), ("r", er, R)):
        kk = torch.empty((B, cap * 28), dtype=torch.uint8, device=DEV)
        dd = torch.empty((B, cap, 32), dtype=torch.uint8, device=DEV)
        nn = torch.empty(B, dtype=torch.int32, device=DEV)
        e.extract_batch_device(X.data_ptr(), B, W, H, W, W * H, kk.data_ptr(), cap, dd.data_ptr(),
                               nn.data_ptr())
        bufs[side] = (kk, dd, nn)
    ur = torch.empty((B, cap), dtype=torch.float32, device=DEV)
    dp = torch.empty((B, cap), dtype=torch.float32, device=DEV)
    (kl, dl, nl), (kr, dr, nr) = bufs["l"], bufs["r"]

    def go():
        el.compute_stereo_matches_device(er, B, kl.data_ptr(), dl.data_ptr(), nl.data_ptr(),
                                         kr.data_ptr(), dr.data_ptr(), nr.data_ptr(), cap, 50.0,
                                         0.1, ur.data_ptr(), dp.data_ptr())
    t = timed(go, 20)
    p = oracle.params(1000, 1.2, 8, 20, 7)
    a, b = pairs[0]
    okl, odl = oracle.extract(p, a)
    okr, odr = oracle.extract(p, b)
    tc = cpu_timed(lambda: oracle.compute_stereo_matches(p, a, b, okl, odl, okr, odr, 50.0, 0.1))
    nkp = float(nl.float().mean())
    emit("(f)2 stereo ComputeStereoMatches (640x480, 1000 kp per side)", "pairs/s", B, t, tc,
         B * nkp * (2 * 60 + 121 + 231 + 8), "device batch of 128 rectified pairs, pyramids of "
         "both extractors resident; bytes = keypoints + descriptors of both sides + the two SAD "
         "windows + outputs per left keypoint; the CPU leg (oracle) also rebuilds both pyramids "
         "per call, which the reference gets from its extractors", cpu_units=1)
    # the per-frame call (Frame.cc:82): one pair through the host ABI, on batch frame 0's pyramids
    t1 = timed(lambda: el.ComputeStereoMatches(er, okl, odl, okr, odr, 50.0, 0.1, frame=0), 100)
    emit("(f)2 stereo ComputeStereoMatches of one pair (host ABI, 640x480, 1000 kp per side)",
         "pairs/s", 1, t1, tc, nkp * (2 * 60 + 121 + 231 + 8),
         "host ABI: keypoints and descriptors of both sides in by one DMA from a pinned block, "
         "u_right | depth | status back by one; the extractors' pyramids resident", cpu_units=1)
    el.close()
    er.close()


def row_reloc():
    import scenarios as S
    c = S.sbp_keyframe_case(0)
    m = native.ORBmatcher(0.9, True, device=0)

    def go():
        m.SearchByProjectionKeyFrame(c["cur"], c["tcw_cur"], c["cam"], c["log_scale"],
                                     c["kf_angle"], c["kf_valid"], c["kf_bad"], c["found"],
                                     c["kf_xyz"], c["kf_desc"], c["kf_min"], c["kf_max"], 10, 100,
                                     frame_mp=c["frame_mp"], kf_ids=c["kf_ids"])
    t = timed(go, 50)
    tc = cpu_timed(lambda: oracle.search_by_projection_keyframe(c, 10, 100))
    n = len(c["kf_valid"])
    emit("(f)3 relocalisation SearchByProjection(Frame&, KeyFrame*) (1000-point keyframe)",
         "calls/s", 1, t, tc, n * (12 + 32 + 8 + 4 + 3) + c["cur"].n * 60,
         "host ABI (uploads included): latency-bound, 5 launches (scatter, grid, fixed-slot "
         "candidates, one-workgroup resolver, gather) and one wait on a done word")
    m.close()


def row_fuse():
    """ORBmatcher::Fuse's search (ORBmatcher.cc:828-978): the host form for one keyframe (about
    1,300 points) and the device batch LocalMapping::SearchInNeighbors makes of it (20 neighbour
    keyframes against the same points).  No CPU leg: the oracle has no Fuse port."""
    import fuse_cases as FC
    c = FC.fuse_case(0)
    kf, n_mp = c["kf"], len(c["xyz"])
    m = native.ORBmatcher(0.6, True, device=0)
    args = (kf, c["tcw"], c["cam"], c["log_scale"], c["inv_sigma2"], c["xyz"], c["normal"],
            c["min_dist"], c["max_dist"], c["desc"], 3.0, FC.SE3)
    nf = m.FuseSearch(*args, skip=c["skip"])[2]
    t = timed(lambda: m.FuseSearch(*args, skip=c["skip"]), 100)
    per_pt = 12 + 12 + 8 + 32 + 1 + 8
    line = {"row": f"Fuse search, one keyframe (host ABI, {n_mp} points, {kf.n} kp, SE3 th 3)",
            "unit": "calls/s", "value": round(1 / t, 2), "ms_per_call": round(t * 1e3, 4),
            "units_per_call": 1, "bytes_per_call": n_mp * per_pt + kf.n * 64, "n_found": nf,
            "cpu_value": None, "note": "host ABI (uploads included): scatter, grid, search, gather; "
            "one wait on a done word; no CPU leg (the oracle has no Fuse port)"}
    print(json.dumps(line), flush=True)
    K, cap = 20, kf.n
    rng = np.random.Generator(np.random.PCG64(3))
    poses = np.stack([c["tcw"]] + [FC.S.pose(rng, 0.002, 0.01) for _ in range(K - 1)])
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(DEV)  # noqa: E731
    d_keys, d_desc, d_ur = up(np.tile(kf.keys, K)), up(np.tile(kf.desc, (K, 1))), up(np.tile(kf.u_right, K))
    d_n = up(np.full(K, kf.n, np.int32))
    d_pts = [up(c[k]) for k in ("xyz", "normal", "min_dist", "max_dist", "desc")]
    d_skip = up(np.tile(c["skip"], K))
    d_bi = torch.empty(K * n_mp, dtype=torch.int32, device=DEV)
    d_bd = torch.empty(K * n_mp, dtype=torch.int32, device=DEV)
    d_st = torch.empty(1, dtype=torch.int32, device=DEV)
    m.set_stream(torch.cuda.current_stream(DEV).cuda_stream)

    def go():
        m.fuse_search_batch_device(K, d_keys.data_ptr(), cap, d_desc.data_ptr(), cap * 32,
                                   d_ur.data_ptr(), cap, d_n.data_ptr(), poses, c["cam"],
                                   (0.0, 640.0, 0.0, 480.0), kf.scale_factors, c["inv_sigma2"],
                                   c["log_scale"], n_mp, *(x.data_ptr() for x in d_pts),
                                   d_skip.data_ptr(), 3.0, FC.SE3, d_bi.data_ptr(), d_bd.data_ptr(),
                                   d_st.data_ptr())
    t = timed(go, 100)
    assert int(d_st[0]) == 0 and int((d_bi.view(K, n_mp)[0] >= 0).sum()) == nf
    line = {"row": f"Fuse search, device batch ({K} keyframes x {n_mp} points, {kf.n} kp each, SE3 th 3)",
            "unit": "keyframes/s", "value": round(K / t, 2), "ms_per_call": round(t * 1e3, 4),
            "units_per_call": K, "bytes_per_call": K * (n_mp * (per_pt + 8) + kf.n * 64),
            "matches": int((d_bi >= 0).sum()), "cpu_value": None,
            "note": "device form, everything resident: one memset, one grid launch (a workgroup per "
            "keyframe), one search launch (a wave per pair); no CPU leg"}
    print(json.dumps(line), flush=True)
    m.close()


def row_triangulation():
    """ORBmatcher::SearchForTriangulation (ORBmatcher.cc:660-826): the host form for one pair and
    the device batch LocalMapping::CreateNewMapPoints makes of it (one keyframe against 20
    neighbours, about 1,000 keypoints each, FeatureVectors at levelsup 4 of the synthetic
    vocabulary, written on the device by the batched transform), issued back to back; beside it
    SearchByBoW's batch at the same slot shape (the closest kernel in structure).  No CPU leg: the
    oracle has no port of this matcher."""
    import ctypes as C
    import scenarios as S
    kf = S.extract_frame(0, 1000, ini=20)
    shifts = [(1 + s % 5, -(s % 3)) for s in range(20)]
    cache = {}
    nbr = [cache.setdefault(sh, S.extract_frame(0, 1000, shift=sh, ini=20)) for sh in shifts]
    parent, word, desc, weight = vocab_arrays(10, 6, 0, anchors=kf.desc[::97])
    st = C.c_int(0)
    h = native.lib().orbfe_vocabulary_create(10, 6, 0, 0, len(parent), native.ptr(parent),
                                             native.ptr(word), native.ptr(desc), native.ptr(weight), 0,
                                             C.byref(st))
    assert h, st.value
    gv = native.Vocabulary.__new__(native.Vocabulary)
    gv._h = C.c_void_p(h)
    stream = torch.cuda.current_stream(DEV).cuda_stream
    gv.set_stream(stream)
    frames = [kf] + nbr
    B, cap, P = len(frames), 1100, len(nbr)
    dd = np.zeros((B, cap, 32), np.uint8)
    kk = np.zeros((B, cap), native.KEYPOINT_DTYPE)
    ang = np.zeros((B, cap), np.float32)
    for i, x in enumerate(frames):
        dd[i, :x.n], kk[i, :x.n], ang[i, :x.n] = x.desc, x.keys, x.keys["angle"]
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(DEV)  # noqa: E731
    D, Kp, A = up(dd), up(kk), up(ang)
    N = up(np.array([x.n for x in frames], np.int32))
    wid = torch.empty((B, cap), dtype=torch.int32, device=DEV)
    val = torch.empty((B, cap), dtype=torch.float64, device=DEV)
    nid = torch.empty((B, cap), dtype=torch.int32, device=DEV)
    off = torch.empty((B, cap + 1), dtype=torch.int32, device=DEV)
    feat = torch.empty((B, cap), dtype=torch.int32, device=DEV)
    nw = torch.empty(B, dtype=torch.int32, device=DEV)
    nn = torch.empty(B, dtype=torch.int32, device=DEV)
    gv.transform_batch_device(B, D.data_ptr(), N.data_ptr(), cap, 4, wid.data_ptr(), val.data_ptr(),
                              nw.data_ptr(), nid.data_ptr(), off.data_ptr(), feat.data_ptr(),
                              nn.data_ptr())
    torch.cuda.synchronize()
    scale = kf.scale_factors
    sigma2 = (scale * scale).astype(np.float32)
    # neighbour s is the keyframe's image rolled by (dy, dx): y2 = y1 + dy, the epipolar lines of a
    # sideways motion (a = 0, b = 1, c = -y1 - dy); the epipole far outside the image
    f12 = np.stack([np.array([[0, 0, 0], [0, 0, -1], [0, 1, -dy]], np.float32) for dy, _ in shifts])
    epi = np.tile(np.array([-5000, -5000], np.float32), (P, 1))
    fvs = []
    for i in (0, 1):
        k = int(nn[i])
        o = off[i, :k + 1].cpu().numpy()
        fvs.append((nid[i, :k].cpu().numpy(), o, feat[i, :o[-1]].cpu().numpy()))
    m = native.ORBmatcher(0.6, False, device=0)   # LocalMapping.cc:212
    none = [np.zeros(x.n, np.uint8) for x in frames[:2]]
    hargs = (frames[0], none[0], fvs[0], frames[1], none[1], fvs[1], f12[0], epi[0], sigma2)
    n_host = m.SearchForTriangulation(*hargs)[1]
    t = timed(lambda: m.SearchForTriangulation(*hargs), 100)
    per_pair = (frames[0].n + frames[1].n) * (32 + 28 + 1 + 4)
    line = {"row": f"SearchForTriangulation, one pair (host ABI, {frames[0].n} x {frames[1].n} kp, "
            f"{len(fvs[0][0])} nodes)", "unit": "calls/s", "value": round(1 / t, 2),
            "ms_per_call": round(t * 1e3, 4), "units_per_call": 1, "bytes_per_call": per_pair,
            "nmatches": n_host, "cpu_value": None,
            "note": "host ABI (uploads included): scatter, init, search, gather; one wait on a done "
            "word; no CPU leg (the oracle has no port of this matcher)"}
    print(json.dumps(line), flush=True)
    m.set_stream(stream)
    p1 = torch.zeros(P, dtype=torch.int32, device=DEV)
    p2 = torch.arange(1, P + 1, dtype=torch.int32, device=DEV)
    dF, dE = up(f12), up(epi)
    mp = torch.zeros(B * cap, dtype=torch.uint8, device=DEV)
    out = torch.empty((P, cap), dtype=torch.int32, device=DEV)
    nmv = torch.empty(P, dtype=torch.int32, device=DEV)
    stv = torch.empty(1, dtype=torch.int32, device=DEV)

    def go():
        m.search_for_triangulation_batch_device(
            cap, Kp.data_ptr(), D.data_ptr(), None, mp.data_ptr(), N.data_ptr(), nn.data_ptr(),
            nid.data_ptr(), off.data_ptr(), feat.data_ptr(), P, p1.data_ptr(), p2.data_ptr(),
            dF.data_ptr(), dE.data_ptr(), scale, sigma2, out.data_ptr(), nmv.data_ptr(), stv.data_ptr())
    t = timed(go, 100)
    assert int(stv[0]) == 0 and int(nmv[0]) == n_host
    line = {"row": f"SearchForTriangulation, device batch (1 keyframe x {P} neighbours, ~{kf.n} kp each, "
            "levelsup 4)", "unit": "pairs/s", "value": round(P / t, 2), "ms_per_call": round(t * 1e3, 4),
            "us_per_pair": round(t * 1e6 / P, 3), "units_per_call": P, "bytes_per_call": P * per_pair,
            "matches": int(nmv.sum()), "cpu_value": None,
            "note": "device form, FeatureVectors as the batched transform wrote them; 2 launches (init; "
            "search, a wave per common node); issued back to back; no CPU leg"}
    print(json.dumps(line), flush=True)
    # SearchByBoW's batch at the same slot shape: the 20 neighbours as keyframes (every feature
    # with a map point) against the keyframe as the frame
    mb = native.ORBmatcher(0.75, True, device=0)
    mb.set_stream(stream)
    ok = torch.ones(B * cap, dtype=torch.uint8, device=DEV)

    def gob():
        mb.search_by_bow_batch_device(P, p2.data_ptr(), p1.data_ptr(), cap, D.data_ptr(), A.data_ptr(),
                                      ok.data_ptr(), nn.data_ptr(), nid.data_ptr(), off.data_ptr(),
                                      feat.data_ptr(), cap, D.data_ptr(), A.data_ptr(), nn.data_ptr(),
                                      nid.data_ptr(), off.data_ptr(), feat.data_ptr(), out.data_ptr(),
                                      nmv.data_ptr(), stv.data_ptr())
    tb = timed(gob, 100)
    assert int(stv[0]) == 0
    line = {"row": f"SearchByBoW, device batch at the same slot shape ({P} pairs, ~{kf.n} features)",
            "unit": "pairs/s", "value": round(P / tb, 2), "ms_per_call": round(tb * 1e3, 4),
            "us_per_pair": round(tb * 1e6 / P, 3), "units_per_call": P,
            "bytes_per_call": P * (frames[0].n + frames[1].n) * (32 + 8), "matches": int(nmv.sum()),
            "cpu_value": None, "triangulation_over_bow": round(t / tb, 3),
            "note": "the comparison row for SearchForTriangulation's batch: same slots, same grid shape"}
    print(json.dumps(line), flush=True)
    m.close()
    mb.close()
    gv.close()


def row_track():
    """The per-frame tracking-loop matchers through the host ABI (uploads included):
    TrackWithMotionModel's SearchByProjection(CurrentFrame, LastFrame, th, mono)
    (Tracking.cc:1132, ORBmatcher.cc:1331-1473) and MonocularInitialization's
    SearchForInitialization (Tracking.cc:844, ORBmatcher.cc:408-523)."""
    import scenarios as S
    c = S.sbp_last_case(0)
    args = (c["cur"], c["tcw_cur"], c["cam"], c["last_keys"], c["last_valid"], c["last_outlier"],
            c["last_xyz"], c["last_desc"], c["last_nobs"], c["tcw_last"])
    m = native.ORBmatcher(0.9, True, device=0)
    t = timed(lambda: m.SearchByProjectionLast(*args, 15.0, True, last_ids=c["last_ids"]), 50)
    tc = cpu_timed(lambda: oracle.search_by_projection_last(*args, 15.0, True, True,
                                                            last_ids=c["last_ids"]))
    n = len(c["last_valid"])
    emit("tracking SearchByProjection(CurrentFrame, LastFrame) (1000 kp each, mono th 15)",
         "calls/s", 1, t, tc, n * (12 + 32 + 28 + 8) + c["cur"].n * 60,
         "host ABI (uploads included): one call per tracked frame, latency-bound (fixed-slot "
         "candidates, one wait on a done word)")
    m.close()
    # TrackLocalMap's SearchByProjection(Frame&, vector<MapPoint*>, th) (Tracking.cc:1283,
    # ORBmatcher.cc:38-131) through the host ABI, isInFrustum's outputs given, 2000 map points
    f, mps, fmp, fobs, ids = S.sbp_local_case(0, 2000)
    m = native.ORBmatcher(0.8, True, device=0)
    t = timed(lambda: m.SearchByProjection(f, mps, 3.0, fmp, fobs, ids), 50)
    tc = cpu_timed(lambda: oracle.search_by_projection_local(f, mps, 3.0, 0.8, fmp, fobs, ids))
    emit("tracking SearchByProjection(Frame&, local map points) (2000 points, th 3)", "calls/s", 1,
         t, tc, 2000 * (32 + 24) + f.n * 60,
         "host ABI (uploads included): fixed-slot candidates, one-workgroup resolver, one wait")
    m.close()
    f1, f2, prev = S.sfi_case(0)
    m = native.ORBmatcher(0.9, True, device=0)
    t = timed(lambda: m.SearchForInitialization(f1, f2, prev, 100), 20)
    tc = cpu_timed(lambda: oracle.search_for_initialization(f1, f2, prev, 100, 0.9, True))
    emit("initialization SearchForInitialization(F1, F2, window 100) (2000 kp each)", "calls/s",
         1, t, tc, (f1.n + f2.n) * 60,
         "host ABI (uploads included): sequential greedy with steals, one wave resolves it")
    m.close()


def row_distinctive():
    from test_distinctive import make_case
    off, desc = make_case(3, n_mp=50_000, max_obs=20)
    m = native.ORBmatcher(device=0)
    d_off = torch.from_numpy(off).to(DEV)
    d_desc = torch.from_numpy(desc).to(DEV)
    best = torch.empty(len(off) - 1, dtype=torch.int32, device=DEV)
    out = torch.empty((len(off) - 1, 32), dtype=torch.uint8, device=DEV)
    m.set_stream(torch.cuda.current_stream(DEV).cuda_stream)
    import ctypes as C
    L = native.lib()

    def go():
        L.orbfe_distinctive_descriptors_device(m._h, len(off) - 1, C.c_void_p(d_off.data_ptr()),
                                               C.c_void_p(d_desc.data_ptr()),
                                               C.c_void_p(best.data_ptr()),
                                               C.c_void_p(out.data_ptr()))
    t = timed(go, 20)
    sub = 2000
    tc = cpu_timed(lambda: oracle.distinctive_descriptors(off[:sub + 1], desc[:off[sub]])) * (len(off) - 1) / sub
    emit("(f)4 ComputeDistinctiveDescriptors (50k map points, 0-20 observations)", "points/s",
         len(off) - 1, t, tc, len(desc) * 32 + (len(off) - 1) * 40,
         "device form; CPU time scaled from a 2000-point sample")
    m.close()


def vocab_arrays(k=10, L=6, seed=0, anchors=None):
    """A complete k-ary tree of depth L as node arrays (vectorised synthetic ORBvoc stand-in)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    parent, desc, word, weight = [np.zeros(1, np.int32)], [np.zeros((1, 32), np.uint8)], [np.zeros(1, np.uint8)], [np.zeros(1)]
    prev = np.zeros(1, np.int64)
    prev_desc = np.zeros((1, 32), np.uint8)
    nid = 1
    for level in range(1, L + 1):
        cnt = len(prev) * k
        par = np.repeat(prev, k)
        if level == 1:
            d = anchors[np.arange(cnt) % len(anchors)] if anchors is not None else rng.integers(0, 256, (cnt, 32), dtype=np.uint8)
        else:
            bits = np.unpackbits(np.repeat(prev_desc, k, axis=0), axis=1)
            bits ^= (rng.uniform(size=bits.shape) < 0.12).astype(np.uint8)
            d = np.packbits(bits, axis=1)
        leaf = level == L
        parent.append(par.astype(np.int32))
        desc.append(d)
        word.append(np.full(cnt, int(leaf), np.uint8))
        w = np.where(rng.uniform(size=cnt) < 0.03, 0.0, rng.uniform(0.5, 8.0, cnt)) if leaf else np.zeros(cnt)
        weight.append(w)
        prev = np.arange(nid, nid + cnt)
        prev_desc = d
        nid += cnt
    return (np.concatenate(parent), np.concatenate(word), np.ascontiguousarray(np.concatenate(desc)),
            np.concatenate(weight).astype(np.float64))


def row_bow(tmpdir):
    import ctypes as C
    import scenarios as S
    f0 = S.extract_frame(0, 1000, ini=20)
    parent, word, desc, weight = vocab_arrays(10, 6, 0, anchors=f0.desc[::97])
    L = native.lib()
    st = C.c_int(0)
    h = L.orbfe_vocabulary_create(10, 6, 0, 0, len(parent), native.ptr(parent), native.ptr(word),
                                  native.ptr(desc), native.ptr(weight), 0, C.byref(st))
    assert h, st.value
    gv = native.Vocabulary.__new__(native.Vocabulary)
    gv._h = C.c_void_p(h)
    gv.set_stream(torch.cuda.current_stream(DEV).cuda_stream)
    B, cap = 256, 1100
    fr = [S.extract_frame(s, 1000, ini=20) for s in range(8)]
    dd = np.zeros((B, cap, 32), np.uint8)
    nn = np.zeros(B, np.int32)
    for i in range(B):
        x = fr[i % 8]
        dd[i, :x.n] = x.desc
        nn[i] = x.n
    D, N = torch.from_numpy(dd).to(DEV), torch.from_numpy(nn).to(DEV)
    o = [torch.empty((B, cap), dtype=t, device=DEV) for t in (torch.int32, torch.float64, torch.int32)]
    off = torch.empty((B, cap + 1), dtype=torch.int32, device=DEV)
    feat = torch.empty((B, cap), dtype=torch.int32, device=DEV)
    cnt = [torch.empty(B, dtype=torch.int32, device=DEV) for _ in range(2)]

    def go():
        gv.transform_batch_device(B, D.data_ptr(), N.data_ptr(), cap, 4, o[0].data_ptr(),
                                  o[1].data_ptr(), cnt[0].data_ptr(), o[2].data_ptr(),
                                  off.data_ptr(), feat.data_ptr(), cnt[1].data_ptr())
    t = timed(go, 10)
    path = os.path.join(tmpdir, "voc6.txt")  # the oracle reads the text format
    with open(path, "w") as fh:
        fh.write("10 6 0 0\n")
        for i in range(1, len(parent)):
            fh.write(f"{parent[i]} {int(word[i])} " + " ".join(map(str, desc[i].tolist())) +
                     f" {float(weight[i])!r}\n")
    ov = oracle.Vocabulary(path)
    assert ov.words == int(word.sum()) and len(ov.transform(fr[0].desc, 4)[0]) > 100
    tc = cpu_timed(lambda: ov.transform(fr[0].desc, 4))
    # per descriptor: k=10 children x 6 levels x 32 B of node descriptors + its own 32 B;
    # per kept feature ~24 B of BowVector / FeatureVector output
    nb = B * 1000 * (60 * 32 + 32 + 24)
    emit("(f)4 BoW transform, ComputeBoW (k=10 L=6 1.1M-node vocabulary, 1000 desc)",
         "frames/s", B, t, tc, nb, "device batch of 256 frames; synthetic vocabulary of ORBvoc's "
         "shape (ORBvoc.txt absent)", cpu_units=1)
    # the per-keyframe call (Frame::ComputeBoW) through the host ABI
    t1 = timed(lambda: gv.transform(fr[0].desc, 4), 100)
    emit("(f)4 BoW transform, ComputeBoW of one frame (host ABI, 1000 desc, same vocabulary)",
         "frames/s", 1, t1, tc, nb // B, "host ABI: descriptors in and vectors out through one "
         "device-mapped pinned block, one synchronisation")
    kf, f = fr[0], S.extract_frame(0, 1000, shift=(2, -3), ini=20)
    kf_fv = ov.transform(kf.desc, 4)[2:]
    f_fv = ov.transform(f.desc, 4)[2:]
    ok = np.ones(kf.n, np.uint8)
    m = native.ORBmatcher(0.75, True, device=0)
    t = timed(lambda: m.SearchByBoW(kf.desc, kf.keys["angle"], ok, kf_fv, f.desc, f.keys["angle"], f_fv), 50)
    tc = cpu_timed(lambda: oracle.search_by_bow(kf.desc, kf.keys["angle"], ok, kf_fv, f.desc,
                                                f.keys["angle"], f_fv, 0.75, True))
    emit("(f)4 SearchByBoW(KeyFrame*, Frame&) (1000 x 1000 features, level-2 nodes)", "calls/s",
         1, t, tc, (kf.n + f.n) * (32 + 8), "host ABI (uploads included), latency-bound: one "
         "workgroup per common node, the host waits on the output slots")
    # Tracking::Relocalization's candidate loop (Tracking.cc:1636-1656) as one device call:
    # the current frame against P candidate keyframes, everything resident in HBM
    from test_bow import pack_slots
    P, kcap = 64, 1100
    kfr = [S.extract_frame(s, 1000, shift=(s % 5, -(s % 3)), ini=20) for s in range(8)]
    rng = np.random.Generator(np.random.PCG64(1))
    items = [(x.desc, x.keys["angle"], (rng.uniform(size=x.n) < 0.8).astype(np.uint8),
              ov.transform(x.desc, 4)[2:]) for x in kfr]
    K = [torch.from_numpy(x).to(DEV) for x in pack_slots(items, kcap)]
    F = [torch.from_numpy(x).to(DEV) for x in pack_slots([(f.desc, f.keys["angle"],
                                                           np.ones(f.n, np.uint8), f_fv)], kcap)]
    pk = torch.arange(P, dtype=torch.int32, device=DEV) % len(items)
    pf = torch.zeros(P, dtype=torch.int32, device=DEV)
    out = torch.empty((P, kcap), dtype=torch.int32, device=DEV)
    nmv = torch.empty(P, dtype=torch.int32, device=DEV)
    stv = torch.empty(1, dtype=torch.int32, device=DEV)
    m = native.ORBmatcher(0.75, True, device=0)
    m.set_stream(torch.cuda.current_stream(DEV).cuda_stream)

    def gob():
        m.search_by_bow_batch_device(P, pk.data_ptr(), pf.data_ptr(), kcap, K[0].data_ptr(),
                                     K[1].data_ptr(), K[2].data_ptr(), K[3].data_ptr(),
                                     K[4].data_ptr(), K[5].data_ptr(), K[6].data_ptr(), kcap,
                                     F[0].data_ptr(), F[1].data_ptr(), F[3].data_ptr(),
                                     F[4].data_ptr(), F[5].data_ptr(), F[6].data_ptr(),
                                     out.data_ptr(), nmv.data_ptr(), stv.data_ptr())
    t = timed(gob, 50)
    assert int(stv[0]) == 0
    x = items[1]
    tc = cpu_timed(lambda: oracle.search_by_bow(x[0], x[1], x[2], x[3], f.desc, f.keys["angle"],
                                                f_fv, 0.75, True))
    emit(f"(f)4 SearchByBoW, relocalisation candidate loop (frame vs {P} keyframes, 1000 features)",
         "pairs/s", P, t, tc, P * (kf.n + f.n) * (32 + 8),
         "device batch: one call per relocalisation attempt (Tracking.cc:1636-1656), FeatureVectors "
         "resident; 2 launches (init; search with the orientation filter in each pair's last workgroup)", cpu_units=1)
    m.close()


def jrow(row, unit, units, t, note, **extra):
    line = {"row": row, "unit": unit, "value": round(units / t, 2), "ms_per_call": round(t * 1e3, 4),
            "units_per_call": units, "cpu_value": None, "note": note}
    line.update(extra)
    print(json.dumps(line), flush=True)


def row_loop():
    """The three matchers of LoopClosing::ComputeSim3, each beside the existing row it should
    resemble, measured in the same process: the loop SearchByProjection(pKF, Scw, ...) against the
    relocalisation SearchByProjection (the same driver), SearchBySim3 against two Sim3
    orbfe_fuse_search calls at the same N (it does that work in one launch), SearchByBoW(pKF1,
    pKF2) against SearchByBoW(pKF, F), host form and batch, at the same shapes.  No CPU leg: the
    oracle has no port of these matchers."""
    import fuse_cases as FC
    import loop_cases as LC
    import scenarios as S
    from test_bow import pack_slots
    # -- loop SearchByProjection / relocalisation SearchByProjection
    c = LC.sbp_case(0)
    m = native.ORBmatcher(0.75, True, device=0)
    sargs = (c["kf"], c["tcw"], c["cam"], c["log_scale"], c["xyz"], c["normal"], c["min_dist"],
             c["max_dist"], c["desc"])
    skw = dict(th=10, skip=c["skip"], mp_ids=c["ids"], kf_matched=c["matched0"])
    nm = m.SearchByProjectionSim3(*sargs, **skw)[1]
    t = timed(lambda: m.SearchByProjectionSim3(*sargs, **skw), 100)
    r = S.sbp_keyframe_case(0)
    rargs = (r["cur"], r["tcw_cur"], r["cam"], r["log_scale"], r["kf_angle"], r["kf_valid"],
             r["kf_bad"], r["found"], r["kf_xyz"], r["kf_desc"], r["kf_min"], r["kf_max"], 10, 100)
    rkw = dict(frame_mp=r["frame_mp"], kf_ids=r["kf_ids"])
    m.SearchByProjectionKeyFrame(*rargs, **rkw)
    tr = timed(lambda: m.SearchByProjectionKeyFrame(*rargs, **rkw), 100)
    jrow(f"loop SearchByProjection(pKF, Scw, vpPoints, vpMatched, th 10) (host ABI, {len(c['xyz'])} "
         f"points, {c['kf'].n} kp)", "calls/s", 1, t,
         "host ABI (uploads included): scatter, grid, fixed-slot candidates, resolver, gather; one "
         "wait on a done word", nmatches=nm, rounds=m.last_rounds(),
         comparator_ms=round(tr * 1e3, 4), over_comparator=round(t / tr, 3),
         comparator=f"relocalisation SearchByProjection host form ({len(r['kf_valid'])} points, "
         f"{r['cur'].n} kp, th 10), same process")
    # -- SearchBySim3 / two Sim3 Fuse searches at the same N
    s = LC.sim3_case(0)
    _, _, s1, s2 = LC.masks(s)
    S12, S21 = LC.sim3_mats(s["s12"], s["R12"], s["t12"])
    p1, p2 = s["pts1"], s["pts2"]
    a3 = (s["kf1"], s["kf2"], s["cam1"], s["T1w"], s["T2w"], S12, S21, s["log1"], s["log2"],
          (s1, p1["xyz"], p1["min_dist"], p1["max_dist"], p1["desc"]),
          (s2, p2["xyz"], p2["min_dist"], p2["max_dist"], p2["desc"]))
    nf = m.SearchBySim3(*a3, th=7.5)[3]
    t = timed(lambda: m.SearchBySim3(*a3, th=7.5), 100)
    isg = FC.inv_sigma2()
    s12f = float(s["s12"])

    def fuse_pose(Tsw, Sm, sc):
        """The normalised [R|t] under which Fuse's Sim3 search projects a source keyframe's
        points where SearchBySim3 does; its distance is the world one, 1 / sc times ‖p3Dc‖, so
        the distance bounds are scaled alike and both predict the same levels."""
        Tsw, Sm = Tsw.astype(np.float64), Sm.astype(np.float64)
        R = Sm[:, :3] / sc @ Tsw[:, :3]
        t = (Sm[:, :3] @ Tsw[:, 3] + Sm[:, 3]) / sc
        return np.hstack([R, t[:, None]]).astype(np.float32)
    fa = [(s["kf2"], fuse_pose(s["T1w"], S21, 1.0 / s12f), s["cam1"], s["log2"], isg, p1["xyz"],
           p1["normal"], p1["min_dist"] * np.float32(s12f), p1["max_dist"] * np.float32(s12f),
           p1["desc"], 7.5, FC.SIM3),
          (s["kf1"], fuse_pose(s["T2w"], S12, s12f), s["cam1"], s["log1"], isg, p2["xyz"],
           p2["normal"], p2["min_dist"] / np.float32(s12f), p2["max_dist"] / np.float32(s12f),
           p2["desc"], 7.5, FC.SIM3)]

    def two_fuse():
        return [m.FuseSearch(*a)[2] for a in fa]
    nfuse = two_fuse()
    tf = timed(two_fuse, 100)
    jrow(f"SearchBySim3 (host ABI, {s['kf1'].n} x {s['kf2'].n} features, th 7.5)", "calls/s", 1, t,
         "host ABI (uploads included): scatter, two grids, one search launch for both directions, "
         "the agreement, gather; one wait on a done word", n_found=nf, comparator_found=nfuse,
         comparator_ms=round(tf * 1e3, 4), over_comparator=round(t / tf, 3),
         comparator="two orbfe_fuse_search calls in Sim3 mode on the same keyframes and points "
         "(th 7.5), same process")
    m.close()
    # -- SearchByBoW(pKF1, pKF2) / SearchByBoW(pKF, F): host form, then the batch
    f0 = S.extract_frame(0, 1000, ini=20)
    parent, word, desc, weight = vocab_arrays(10, 6, 0, anchors=f0.desc[::97])
    import ctypes as C
    st = C.c_int(0)
    h = native.lib().orbfe_vocabulary_create(10, 6, 0, 0, len(parent), native.ptr(parent),
                                             native.ptr(word), native.ptr(desc), native.ptr(weight), 0,
                                             C.byref(st))
    assert h, st.value
    ov = native.Vocabulary.__new__(native.Vocabulary)   # the FeatureVectors come from the device
    ov._h = C.c_void_p(h)
    kf, f = f0, S.extract_frame(0, 1000, shift=(2, -3), ini=20)
    kf_fv, f_fv = ov.transform(kf.desc, 4)[2:], ov.transform(f.desc, 4)[2:]
    ok1, ok2 = np.ones(kf.n, np.uint8), np.ones(f.n, np.uint8)
    m = native.ORBmatcher(0.75, True, device=0)
    kk = (kf.desc, kf.keys["angle"], ok1, kf_fv, f.desc, f.keys["angle"], ok2, f_fv)
    kfr = (kf.desc, kf.keys["angle"], ok1, kf_fv, f.desc, f.keys["angle"], f_fv)
    nkk = m.SearchByBoWKeyFrames(*kk)[1]
    t = timed(lambda: m.SearchByBoWKeyFrames(*kk), 100)
    m.SearchByBoW(*kfr)
    tb = timed(lambda: m.SearchByBoW(*kfr), 100)
    jrow(f"SearchByBoW(pKF1, pKF2) (host ABI, {kf.n} x {f.n} features, levelsup 4)", "calls/s", 1, t,
         "host ABI (uploads included): the pair-indexed path with one pair — scatter, init, search "
         "(orientation filter in the last workgroup), gather", nmatches=nkk,
         comparator_ms=round(tb * 1e3, 4), over_comparator=round(t / tb, 3),
         comparator="SearchByBoW(pKF, F) host form on the same two feature sets (its gathered "
         "one-launch path), same process")
    P, cap = 64, 1100
    kfs = [S.extract_frame(q, 1000, shift=(q % 5, -(q % 3)), ini=20) for q in range(8)]
    rng = np.random.Generator(np.random.PCG64(1))
    items = [(x.desc, x.keys["angle"], (rng.uniform(size=x.n) < 0.8).astype(np.uint8),
              ov.transform(x.desc, 4)[2:]) for x in kfs]
    cur = (f.desc, f.keys["angle"], ok2, f_fv)
    K = [torch.from_numpy(x).to(DEV) for x in pack_slots(items + [cur], cap)]
    pk = torch.arange(P, dtype=torch.int32, device=DEV) % len(items)
    pc = torch.full((P,), len(items), dtype=torch.int32, device=DEV)
    pz = torch.zeros(P, dtype=torch.int32, device=DEV)
    out = torch.empty((P, cap), dtype=torch.int32, device=DEV)
    nmv = torch.empty(P, dtype=torch.int32, device=DEV)
    stv = torch.empty(1, dtype=torch.int32, device=DEV)
    m.set_stream(torch.cuda.current_stream(DEV).cuda_stream)
    kp = [x.data_ptr() for x in K]

    def gokk():   # the current keyframe (the last slot) against P candidates
        m.search_by_bow_keyframes_batch_device(P, pc.data_ptr(), pk.data_ptr(), cap, kp[0], kp[1],
                                               kp[2], kp[3], kp[4], kp[5], kp[6], out.data_ptr(),
                                               nmv.data_ptr(), stv.data_ptr())
    t = timed(gokk, 100)
    assert int(stv[0]) == 0
    tot = int(nmv.sum())

    def gokk_swapped():   # the candidates as pKF1: the outer / inner shape of the comparator
        m.search_by_bow_keyframes_batch_device(P, pk.data_ptr(), pc.data_ptr(), cap, kp[0], kp[1],
                                               kp[2], kp[3], kp[4], kp[5], kp[6], out.data_ptr(),
                                               nmv.data_ptr(), stv.data_ptr())
    ts = timed(gokk_swapped, 100)
    assert int(stv[0]) == 0
    F = [x[len(items):].contiguous() for x in K]
    fp = [x.data_ptr() for x in F]

    def gob():    # SearchByBoW's batch: the same candidates as keyframes, the same frame
        m.search_by_bow_batch_device(P, pk.data_ptr(), pz.data_ptr(), cap, kp[0], kp[1], kp[2],
                                     kp[3], kp[4], kp[5], kp[6], cap, fp[0], fp[1], fp[3], fp[4],
                                     fp[5], fp[6], out.data_ptr(), nmv.data_ptr(), stv.data_ptr())
    tb = timed(gob, 100)
    assert int(stv[0]) == 0
    jrow(f"SearchByBoW(pKF1, pKF2), ComputeSim3's candidate loop (keyframe vs {P} candidates, "
         f"~{kf.n} features)", "pairs/s", P, t,
         "device batch, FeatureVectors resident; 2 launches (init; search with the orientation "
         "filter in each pair's last workgroup); issued back to back", matches=tot,
         us_per_pair=round(t * 1e6 / P, 3), comparator_ms=round(tb * 1e3, 4),
         over_comparator=round(t / tb, 3), swapped_ms=round(ts * 1e3, 4),
         swapped_over_comparator=round(ts / tb, 3),
         comparator=f"orbfe_search_by_bow_batch_device on the same slots ({P} pairs), same process")
    m.close()
    ov.close()


def row_kfdb(tmpdir):
    """The keyframe database: one relocalisation query and one loop query (host forms, each with
    its wait) against 2000 keyframes of 1000 words each in the bench vocabulary (k = 10, L = 6),
    words drawn from a 20000-word scene pool so that a query shares ~50 words with a keyframe;
    every keyframe's covisibility list is its 10 predecessors, the loop query's connected set
    the 10 newest keyframes.  Comparator: tests/cpp/kfdb_test --time, a one-thread std::list
    inverted-file walk of the same script on this machine's host.  Two repeats of each."""
    import ctypes as C
    import subprocess
    import kfdb_cases as K
    parent, word, desc, weight = vocab_arrays(10, 6, 0)
    L = native.lib()
    st = C.c_int(0)
    h = L.orbfe_vocabulary_create(10, 6, 0, 0, len(parent), native.ptr(parent), native.ptr(word),
                                  native.ptr(desc), native.ptr(weight), 0, C.byref(st))
    assert h, st.value
    gv = native.Vocabulary.__new__(native.Vocabulary)
    gv._h = C.c_void_p(h)
    nkf, nw = 2000, 1000
    rng = np.random.Generator(np.random.PCG64(11))
    pool = np.sort(rng.choice(10 ** 6, 20000, replace=False)).astype(np.int32)

    def bow():
        ids = np.sort(rng.choice(pool, nw, replace=False)).astype(np.int32)
        v = rng.uniform(0.2, 4.0, nw)
        return ids, v / v.sum()
    db = native.KeyFrameDatabase(gv, 1024, nkf)
    script = []
    for i in range(nkf):
        b = bow()
        script.append(("add", "k%d" % i, *b))
        assert db.add(*b) == i
    for i in range(nkf):
        n = list(range(max(i - 10, 0), i))[::-1]
        script.append(("covis", "k%d" % i, ["k%d" % j for j in n]))
        db.set_covisibility(i, n)
    q = bow()
    conn = list(range(nkf - 10, nkf))
    script += [("reloc", 1, *q), ("loop", 2, *q, ["k%d" % j for j in conn], 0.005)]
    path = os.path.join(tmpdir, "kfdb_script.bin")
    K.dump_script(path, 0, script)
    ncand = [0, 0]
    qid = [10]

    def call():
        qid[0] += 2
        c, _ = db.DetectRelocalizationCandidates(qid[0], *q)
        ncand[0] = len(c)
        c, _ = db.DetectLoopCandidates(qid[0] + 1, *q, conn, 0.005)
        ncand[1] = len(c)
    exe = os.path.join(ROOT, "tests", "cpp", "build", "kfdb_test")
    for rep in range(2):
        t = timed(call, 100, warm=3)
        r = subprocess.run([exe, "--time", path, "20"], capture_output=True, text=True, check=True)
        t_cpu = float(r.stdout.split("ms_per_pass=")[1].split()[0]) * 1e-3
        jrow("kfdb", "query pairs/s", 1, t, f"repeat {rep}: reloc + loop query, {nkf} keyframes x {nw} "
             f"words, candidates {ncand[0]} / {ncand[1]}; comparator: one-thread std::list inverted file",
             comparator_ms=round(t_cpu * 1e3, 4), device_over_comparator=round(t / t_cpu, 3),
             comparator_over_device=round(t_cpu / t, 3))
    db.close()
    gv.close()


def row_rgbd():
    """Frame::ComputeStereoFromRGBD at 640 x 480, ~1000 keypoints per frame: the device batch over
    the slabs the batch extraction wrote, the single-frame host form from the staged depth buffer
    and from a foreign pointer, and the host round trip they replace (D2H of the keypoint slab,
    the lookup in numpy, H2D of mvuRight / mvDepth), which needs nothing of this library but the
    extraction and so runs the same on a build without the RGB-D calls; then the close points."""
    W, H, B = 640, 480, 64
    ex = native.ORBextractor(1000, 1.2, 8, 20, 7, device=0, max_width=W, max_height=H, max_batch=B)
    cap = ex.capacity(W, H)
    imgs = np.stack([synthetic_frame(70 + f % 8, W, H) for f in range(B)])
    r = np.random.default_rng(1)
    depth = r.integers(300, 30000, (B, H, W)).astype(np.uint16)
    depth[r.random(depth.shape) < 0.1] = 0
    factor, bf = np.float32(1.0) / np.float32(5000.0), np.float32(40.0)
    d_img = torch.from_numpy(imgs).to(DEV)
    d_depth = torch.from_numpy(depth.view(np.uint8)).to(DEV)
    d_k = torch.zeros((B, cap * 28), dtype=torch.uint8, device=DEV)
    d_d = torch.zeros((B, cap, 32), dtype=torch.uint8, device=DEV)
    d_n = torch.zeros(B, dtype=torch.int32, device=DEV)
    d_ur = torch.zeros((B, cap), dtype=torch.float32, device=DEV)
    d_dp = torch.zeros((B, cap), dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    ex.extract_batch_device(d_img.data_ptr(), B, W, H, W, W * H, d_k.data_ptr(), cap, d_d.data_ptr(),
                            d_n.data_ptr())
    ex.synchronize()
    cnt = d_n.cpu().numpy()
    nkp = float(cnt.mean())

    def roundtrip(nf):
        k = d_k[:nf].cpu().numpy().view(native.KEYPOINT_DTYPE).reshape(nf, cap)
        c = d_n[:nf].cpu().numpy()
        ur = np.full((nf, cap), -1, np.float32)
        dp = np.full((nf, cap), -1, np.float32)
        for f in range(nf):
            m = int(c[f])
            d = depth[f][k[f, :m]["y"].astype(np.int32), k[f, :m]["x"].astype(np.int32)].astype(np.float32) * factor
            ok = d > 0
            dp[f, :m][ok] = d[ok]
            ur[f, :m][ok] = k[f, :m]["x"][ok] - bf / d[ok]
        d_ur[:nf].copy_(torch.from_numpy(ur))
        d_dp[:nf].copy_(torch.from_numpy(dp))

    shape = f"{W}x{H}, {nkp:.0f} keypoints per frame"
    t = timed(lambda: roundtrip(B), 10)
    jrow("rgbd_roundtrip_batch", "frames/s", B, t,
         f"host round trip, {B} frames ({shape}): D2H keypoint slabs + counts, numpy lookup, H2D mvuRight + mvDepth")
    t = timed(lambda: roundtrip(1), 200)
    jrow("rgbd_roundtrip_single", "frames/s", 1, t, f"host round trip, one frame ({shape})")
    if not hasattr(ex, "compute_stereo_from_rgbd_device"):
        ex.close()
        return
    ref = (d_ur.cpu().numpy().copy(), d_dp.cpu().numpy().copy())

    def dev():
        ex.compute_stereo_from_rgbd_device(B, d_depth.data_ptr(), native.DEPTH_U16, W, H, 2 * W, 2 * W * H,
                                           float(factor), d_k.data_ptr(), d_n.data_ptr(), cap, float(bf),
                                           d_ur.data_ptr(), d_dp.data_ptr())
    t = timed(dev, 200)
    ex.rgbd_status()
    got = (d_ur.cpu().numpy(), d_dp.cpu().numpy())
    same = all(np.array_equal(g[f, :cnt[f]], w[f, :cnt[f]]) for g, w in zip(got, ref) for f in range(B))
    jrow("rgbd_device_batch", "frames/s", B, t,
         f"orbfe_compute_stereo_from_rgbd_device, {B} frames ({shape}), slabs as the extraction wrote them",
         equals_roundtrip=bool(same))
    keys = d_k[0].cpu().numpy().view(native.KEYPOINT_DTYPE)[:cnt[0]].copy()
    buf = ex.depth_buffer(W, H, np.uint16)
    buf[:] = depth[0]
    t = timed(lambda: ex.ComputeStereoFromRGBD(buf, float(factor), keys, float(bf)), 500)
    jrow("rgbd_host_staged", "frames/s", 1, t, f"host form, depth in the handle's buffer, gathered in place ({shape})")
    t = timed(lambda: ex.ComputeStereoFromRGBD(depth[0], float(factor), keys, float(bf)), 200)
    jrow("rgbd_host_foreign", "frames/s", 1, t, f"host form, foreign depth pointer staged first ({shape})")
    # the close points of UpdateLastFrame over the same frames
    mt = native.ORBmatcher(0.9, True, device=0)
    cam = native.Camera(517.3, 516.5, 318.6, 255.3, float(bf), float(bf) / 517.3)
    pose = torch.from_numpy(np.tile(np.asarray([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.float32), (B, 1))).to(DEV)
    d_hp = torch.from_numpy((r.random((B, cap)) < 0.4).astype(np.uint8)).to(DEV)
    o_i = torch.zeros((B, cap), dtype=torch.int32, device=DEV)
    o_c = torch.zeros((B, cap), dtype=torch.uint8, device=DEV)
    o_x = torch.zeros((B, cap, 3), dtype=torch.float32, device=DEV)
    o_f = torch.zeros((2, B, cap), dtype=torch.float32, device=DEV)
    o_n = torch.zeros((4, B), dtype=torch.int32, device=DEV)
    sf = ex.GetScaleFactors()
    torch.cuda.synchronize()

    def close():
        mt.close_points_batch_device(native.CLOSE_SORTED, B, d_k.data_ptr(), d_dp.data_ptr(), d_hp.data_ptr(),
                                     d_n.data_ptr(), cap, cam, pose.data_ptr(), 3.09, 100, sf,
                                     o_i.data_ptr(), o_n[0].data_ptr(), o_c.data_ptr(), o_x.data_ptr(),
                                     o_f[0].data_ptr(), o_f[1].data_ptr(), o_n[1].data_ptr(),
                                     o_n[2].data_ptr(), o_n[3].data_ptr())
    t = timed(close, 200)
    res = o_n.cpu().numpy()
    jrow("close_points_device_batch", "frames/s", B, t,
         f"orbfe_close_points_batch_device, sorted mode, {B} frames ({shape})",
         visited_mean=float(res[0].mean()), status_ok=bool((res[3] == 0).all()))
    hk = keys
    hz = d_dp[0].cpu().numpy()[:cnt[0]].copy()
    hh = d_hp[0].cpu().numpy()[:cnt[0]].copy()
    hp = pose[0].cpu().numpy()
    t = timed(lambda: mt.ClosePoints(native.CLOSE_SORTED, hk, hz, hh, cam, hp, 3.09, sf), 200)
    jrow("close_points_host", "frames/s", 1, t, f"orbfe_close_points host form, sorted mode ({shape})")
    mt.close()
    ex.close()


def row_localmap():
    """Tracking::UpdateLocalMap at the config-5 shape: 1000 frame keypoints (3 in 4 hold a point),
    60 keyframes of 2000 slots each over 50,000 points in a sliding window (neighbours share
    points), ten covisibility neighbours and a parent each; per call orbfe_map_update_local_device
    (a new frame id every call, so every point is listed again) and the gather of the listed
    points into the inputs of orbfe_search_local_points_device.  Comparator: tests/cpp/localmap_test
    --time, the literal std::map loop on one host thread of this machine.  Two repeats."""
    import subprocess
    nkf, per, npts, n = 60, 2000, 50000, 1000
    rng = np.random.default_rng(5)
    lm = native.LocalMap(0, nkf, npts)
    assert lm.add_points(npts) == 0
    for i in range(nkf):
        mps = ((i * (npts - per) // (nkf - 1) + rng.integers(0, per, per)) % npts).astype(np.int32)
        assert lm.add_keyframe(0x7f0000000000 + 0x2c0 * int(rng.integers(1, 1 << 20)) + i, per, mps) == i
        lm.AddObservation(mps, np.full(per, i, np.int32))
    for i in range(nkf):
        lm.UpdateBestCovisibles(i, [(i + j) % nkf for j in range(1, 11)])
        if i:
            lm.set_parent(i, i - 1)
    frame = np.where(rng.uniform(size=n) < 0.75, rng.integers(0, npts, n), -1).astype(np.int32)
    d_frame = torch.from_numpy(frame).to(DEV)
    world = {"xyz": torch.rand((npts, 3), device=DEV), "normal": torch.rand((npts, 3), device=DEV),
             "min_dist": torch.rand(npts, device=DEV), "max_dist": torch.rand(npts, device=DEV),
             "desc": torch.randint(0, 256, (npts, 32), dtype=torch.uint8, device=DEV),
             "n_obs": torch.ones(npts, dtype=torch.int32, device=DEV),
             "skip": torch.zeros(npts, dtype=torch.uint8, device=DEV)}
    out = {k: torch.empty_like(v) for k, v in world.items()}
    out["mp_ids"] = torch.empty(npts, dtype=torch.int32, device=DEV)
    out["bad"] = torch.empty(npts, dtype=torch.uint8, device=DEV)
    src = native.MapPointArrays(**{k: v.data_ptr() for k, v in world.items()})
    dst = native.MapPointArrays(**{k: v.data_ptr() for k, v in out.items()})
    lm.set_stream(torch.cuda.current_stream(DEV).cuda_stream)
    fid, last = [100], [0, 0]

    def update():
        fid[0] += 1
        kfs, _, nmp = lm.update_local_device(fid[0], n, d_frame.data_ptr())
        last[0], last[1] = len(kfs), nmp

    def both():
        update()
        p, cnt = lm.local_points_device()
        lm.gather_points_device(cnt, p, src, dst)
    exe = os.path.join(ROOT, "tests", "cpp", "build", "localmap_test")
    for rep in range(2):
        tu = timed(update, 200, warm=5)
        t = timed(both, 200, warm=5)
        r = subprocess.run([exe, "--time", "50"], capture_output=True, text=True, check=True)
        t_cpu = float(r.stdout.split("ms_per_call=")[1].split()[0]) * 1e-3
        jrow("local_map", "calls/s", 1, t,
             f"repeat {rep}: orbfe_map_update_local_device + gather, {n} frame points, {last[0]} local "
             f"keyframes of {per} slots, {last[1]} local points; comparator: the literal std::map loop, "
             f"one host thread ({r.stdout.strip()})", update_only_ms=round(tu * 1e3, 4),
             gather_ms=round((t - tu) * 1e3, 4), comparator_ms=round(t_cpu * 1e3, 4),
             device_over_comparator=round(t / t_cpu, 3), comparator_over_device=round(t_cpu / t, 3),
             bytes_per_call=int(last[1] * (4 + 72 + 6) + nkf * per * 8))
    lm.close()


def row_covis():
    """KeyFrame::UpdateConnections on the device.  (a) The online call on the config-5 map of
    row_localmap (60 keyframes of 2000 slots over 50,000 points in a sliding window): one keyframe
    per call, every keyframe in turn.  (b) The load-map call (System.cc:188-191): 1000 keyframes
    of 1000 slots over a sliding window in which each shares points with about 20 others, one
    batch call over all of them.  A host clock around calls that end synchronised; comparator:
    tests/cpp/covis_test --time, the literal std::map loop on one host thread of this machine.
    Two repeats."""
    import subprocess

    def world(nkf, per, npts, seed):
        rng = np.random.default_rng(seed)
        lm = native.LocalMap(0, nkf, npts)
        assert lm.add_points(npts) == 0
        for i in range(nkf):
            mps = ((i * (npts - per) // (nkf - 1) + rng.integers(0, per, per)) % npts).astype(np.int32)
            assert lm.add_keyframe(0x7f0000000000 + 0x2c0 * int(rng.integers(1, 1 << 20)) + i, per, mps) == i
            lm.AddObservation(mps, np.full(per, i, np.int32))
        return lm

    exe = os.path.join(ROOT, "tests", "cpp", "build", "covis_test")
    online = world(60, 2000, 50000, 5)
    load = world(1000, 1000, 100000, 6)
    every = np.arange(1000, dtype=np.int32)
    turn = [0]

    def one():
        online.UpdateConnections(turn[0] % 60)
        turn[0] += 1
    for i in range(60):   # as the comparator: every keyframe has been connected once before the clock
        online.UpdateConnections(i)
    for rep in range(2):
        ta = timed(one, 240, warm=5)
        tb = timed(lambda: load.UpdateConnections(every), 10, warm=5)
        r = subprocess.run([exe, "--time", "8"], capture_output=True, text=True, check=True)
        ca, cb = (float(l.split("ms_per_call=")[1].split()[0]) * 1e-3 for l in r.stdout.splitlines()[:2])
        na = float(np.mean([len(online.get_connections(i)[0]) for i in range(60)]))
        nb = float(np.mean([len(load.get_connections(i)[0]) for i in range(0, 1000, 10)]))
        jrow("covis_online", "calls/s", 1, ta,
             f"repeat {rep}: orbfe_map_update_connections, one keyframe of 2000 slots per call, "
             f"{na:.1f} neighbours; comparator: the literal std::map loop, one host thread "
             f"({r.stdout.splitlines()[0]})", comparator_ms=round(ca * 1e3, 4),
             comparator_over_device=round(ca / ta, 3))
        jrow("covis_loadmap", "keyframes/s", 1000, tb,
             f"repeat {rep}: orbfe_map_update_connections, one batch of 1000 keyframes of 1000 slots, "
             f"{nb:.1f} neighbours; comparator: the literal loop ({r.stdout.splitlines()[1]})",
             comparator_ms=round(cb * 1e3, 4), comparator_over_device=round(cb / tb, 3))
    online.close()
    load.close()


def row_culling():
    """LocalMapping::KeyFrameCulling and MapPointCulling on the device.  A seeded map of the
    local-BA kind: 31 keyframes of 1000 slots, 850 of them over 3,300 shared points (observation
    rows of about 8) and 150 private ones, one octave, monocular; the current keyframe lists the
    other 30.  (a) nothing culled: one decide launch; (b) keyframes 10 and 20 have no private
    points and are culled: three decide launches and two SetBadFlags (the map is rebuilt for
    every repeat, outside the clock).  (c) MapPointCulling over 500 recent points, none culled,
    and once with about a third culled.  A host clock around calls that end synchronised;
    comparator: tests/cpp/culling_test --time, the literal loops on one host thread."""
    import subprocess

    def world(full, seed=7):
        rng = np.random.default_rng(seed)
        nkf, per, shared, priv = 31, 1000, 3300, 150
        lm = native.LocalMap(0, nkf, shared + nkf * priv)
        assert lm.add_points(shared + nkf * priv) == 0
        for i in range(nkf):
            mps = rng.integers(0, shared, per).astype(np.int32)
            if i not in full:
                mps[per - priv:] = shared + i * priv + np.arange(priv)
            assert lm.add_keyframe(0x7f0000000000 + 0x2c0 * int(rng.integers(1, 1 << 20)) + i, per, mps) == i
            lm.set_keyframe_features(i, np.zeros(per, np.int32))
            _, first = np.unique(mps, return_index=True)     # a point held twice is observed once
            lm.AddObservation(mps[first], np.full(len(first), i, np.int32), first.astype(np.int32))
        lm.set_ordered_connections(nkf - 1, list(range(1, nkf - 1)) + [0], list(range(nkf - 1, 0, -1)))
        return lm

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        return time.perf_counter() - t0, out

    exe = os.path.join(ROOT, "tests", "cpp", "build", "culling_test")
    r = subprocess.run([exe, "--time", "5"], capture_output=True, text=True, check=True)
    comp = r.stdout.strip().splitlines()
    lm = world(())
    rows = float(np.mean([len(lm.GetObservations(p)[0]) for p in range(0, 3300, 33)]))
    for rep in range(2):
        t = timed(lambda: lm.KeyFrameCulling(30, True, first_kf=0), 50, warm=5)
        assert not lm.KeyFrameCulling(30, True)[1].any()
        jrow("cull_keyframes_none", "calls/s", 1, t,
             f"repeat {rep}: orbfe_map_cull_keyframes, 30 listed keyframes of 1000 slots, rows of {rows:.1f}, "
             f"nothing culled: 1 decide launch, 1 host wait; comparator: {comp[-2]}")
        recent = np.arange(100, 600, dtype=np.int32)
        t = timed(lambda: lm.MapPointCulling(recent, 0, True), 100, warm=5)
        assert len(lm.MapPointCulling(recent, 0, True)[0]) == 500
        jrow("cull_points_none", "calls/s", 1, t,
             f"repeat {rep}: orbfe_map_cull_points, 500 listed points, none culled: 1 launch, 1 host wait; "
             f"comparator: {comp[-1]}")
    ts, culled = [], []
    for rep in range(5):
        w = world((10, 20))
        w.KeyFrameCulling(30, True, kf_slots=[30])        # warm: buffers, code objects
        t, out = clock(lambda: w.KeyFrameCulling(30, True, first_kf=0))
        ts.append(t)
        culled.append(int((out[1] == native.MAP_CULL_CULLED).sum()))
        w.close()
    jrow("cull_keyframes_two", "calls/s", 1, float(np.median(ts)),
         f"orbfe_map_cull_keyframes, the same map with two keyframes culled ({culled}): 3 decide launches and "
         f"2 SetBadFlags; median of 5 single calls on fresh maps, min {min(ts) * 1e3:.3f} max {max(ts) * 1e3:.3f} ms; "
         f"comparator: {comp[-2]}")
    lm.set_point_counters(np.arange(100, 600, 3, dtype=np.int32), found=np.zeros(167, np.int32),
                          visible=np.full(167, 5, np.int32))
    t, out = clock(lambda: lm.MapPointCulling(np.arange(100, 600, dtype=np.int32), 0, True))
    jrow("cull_points_third", "calls/s", 1, t,
         f"orbfe_map_cull_points, 500 listed points, {len(out[1])} culled: 2 launches, 2 host waits; one call")
    lm.close()


if __name__ == "__main__":
    import tempfile
    with tempfile.TemporaryDirectory() as td:
        rows = {"single": row_single, "color": row_color, "stereo": row_stereo, "reloc": row_reloc, "fuse": row_fuse, "triangulation": row_triangulation, "track": row_track,
                "distinctive": row_distinctive, "bow": lambda: row_bow(td),
                "loop": row_loop, "kfdb": lambda: row_kfdb(td), "rgbd": row_rgbd,
                "localmap": row_localmap, "covis": row_covis, "culling": row_culling}
        for name in (sys.argv[1:] or list(rows)):
            rows[name]()
