"""The RGB-D kernels (orbfe_rgbd.hip) against the restatement of rgbd_cases.py: every output
compares on its float bits.  (A NaN compares as NaN: which of its payloads an inf * 0 or an
inf - inf produces is not IEEE's to say, and the reference stores whatever its FPU gives.)"""
import numpy as np
import pytest

import rgbd_cases as R
from orbslam_mapsave_amd import abi, native

pytestmark = pytest.mark.gpu
F32 = np.float32
SENT = F32(-77.5)
STEREO = R.stereo_cases()
CLOSE = R.close_cases()
CAMERA = abi.Camera(*(float(c) for c in R.CAM), float(R.BF), float(R.BF / R.CAM[0]))
EXTRACTOR = (1000, 1.2, 8, 20, 7)


def bits(a):
    a = np.ascontiguousarray(a)
    if a.dtype != F32:
        return a.tobytes()
    u = a.view(np.uint32).copy()
    u[np.isnan(a)] = 0x7FC00000
    return u.tobytes()


def assert_same(got, want, what):
    for k in want:
        g, w = got[k], want[k]
        if w is None or np.isscalar(w):
            assert g == w, (what, k, g, w)
        else:
            assert g.shape == w.shape and g.dtype == w.dtype and bits(g) == bits(w), (what, k, g, w)


@pytest.fixture(scope="module")
def ex():
    return native.ORBextractor(*EXTRACTOR, device=0, max_width=640, max_height=480, max_batch=5)


@pytest.fixture(scope="module")
def matcher():
    return native.ORBmatcher(0.9, True, device=0)


@pytest.fixture(scope="module")
def dev():
    import torch
    return torch.device("cuda", 0)


def up(a, dev):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:  # torch has no arithmetic on uint16; the bytes are what travels
        a = a.view(np.uint8)
    return torch.from_numpy(a.view(np.uint8) if a.dtype.fields else a).to(dev)


# ---- ComputeStereoFromRGBD ---------------------------------------------------------------------

def stereo_want(c):
    ur, dp, st = R.restated_stereo(*c)
    return {"u_right": ur, "depth": dp, "status": st}


def stereo_host(ex, c, img=None):
    im, factor, keys, keys_un, bf = c
    ur, dp, st = ex.ComputeStereoFromRGBD(im if img is None else img, float(factor), keys, float(bf),
                                          keys_un, results=True)
    return {"u_right": ur, "depth": dp, "status": st}


@pytest.mark.parametrize("name", sorted(STEREO))
def test_stereo_host_form(ex, name):
    assert_same(stereo_host(ex, STEREO[name]), stereo_want(STEREO[name]), name)


def test_stereo_raises_on_out_of_image_keypoint(ex):
    im, factor, keys, keys_un, bf = STEREO["edges_out"]
    with pytest.raises(abi.OrbfeError) as e:
        ex.ComputeStereoFromRGBD(im, float(factor), keys, float(bf))
    assert e.value.status == abi.ORBFE_ERR_UNSUPPORTED


@pytest.mark.parametrize("name", ["u16_n257", "f32_n257", "edges_out", "keys_un_distinct"])
def test_stereo_routes_agree(ex, name, monkeypatch):
    """The staged depth buffer (gathered in place), a foreign pointer (copied in) and the same
    two with ORBFE_ZERO_COPY=0 give identical outputs."""
    c = STEREO[name]
    want = stereo_want(c)
    h, w = c[0].shape
    monkeypatch.setenv("ORBFE_ZERO_COPY", "0")
    plain = native.ORBextractor(*EXTRACTOR, device=0, max_width=640, max_height=480)
    monkeypatch.delenv("ORBFE_ZERO_COPY")
    for e in (ex, plain):
        buf = e.depth_buffer(w, h, c[0].dtype)
        assert buf.shape == (h, w) and buf.dtype == c[0].dtype
        buf[:] = c[0]
        assert_same(stereo_host(e, c, buf), want, (name, "staged"))
        assert e.depth_buffer(w, h, c[0].dtype).ctypes.data == buf.ctypes.data
        assert_same(stereo_host(e, c), want, (name, "foreign"))
        # a staged frame survives a foreign call in between
        assert_same(stereo_host(e, c, buf), want, (name, "staged again"))
    plain.close()


@pytest.mark.parametrize("n_frames", [1, 2, 5])
def test_stereo_batch_device(ex, dev, n_frames):
    """Unequal counts with an empty frame, a loose kps_cap, distinct keys_un, padded planes; the
    slots at and past a frame's count keep what they held."""
    import torch
    r = np.random.default_rng(20 + n_frames)
    w, h, stride = 97, 61, 2 * 104
    counts = [65, 0, 257, 1, 64][:n_frames]
    cap = max(counts) + 37
    planes = r.integers(0, 65536, (n_frames, h + 2, stride // 2)).astype(np.uint16)
    planes[r.random(planes.shape) < 0.2] = 0
    slab = np.zeros((n_frames, cap), abi.KEYPOINT_DTYPE)
    slab_un = np.zeros((n_frames, cap), abi.KEYPOINT_DTYPE)
    want = []
    for f, n in enumerate(counts):
        k = R.keys_at(r.random(cap).astype(F32) * F32(w - 1), r.random(cap).astype(F32) * F32(h - 1))
        if f == 2:
            k["x"][5], k["y"][9] = F32(w), F32(h)  # out of the image: -1 / -1, neighbours exact
        ku = k.copy()
        ku["x"] += F32(1.5)
        slab[f], slab_un[f] = k, ku
        want.append(R.restated_stereo(planes[f, :h, :w], R.FACTOR_5000, k[:n], ku[:n], R.BF))
    d_depth, d_k, d_ku = up(planes, dev), up(slab, dev), up(slab_un, dev)
    d_n = up(np.asarray(counts, np.int32), dev)
    d_ur = torch.full((n_frames, cap), float(SENT), dtype=torch.float32, device=dev)
    d_dp = torch.full((n_frames, cap), float(SENT), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    ex.compute_stereo_from_rgbd_device(n_frames, d_depth.data_ptr(), native.DEPTH_U16, w, h, stride,
                                       (h + 2) * stride, float(R.FACTOR_5000), d_k.data_ptr(),
                                       d_n.data_ptr(), cap, float(R.BF), d_ur.data_ptr(), d_dp.data_ptr(),
                                       d_keys_un=d_ku.data_ptr())
    if n_frames > 2:
        with pytest.raises(abi.OrbfeError) as e:
            ex.rgbd_status()
        assert e.value.status == abi.ORBFE_ERR_UNSUPPORTED
    else:
        ex.rgbd_status()
    ur, dp = d_ur.cpu().numpy(), d_dp.cpu().numpy()
    for f, n in enumerate(counts):
        assert bits(ur[f, :n]) == bits(want[f][0]) and bits(dp[f, :n]) == bits(want[f][1]), f
        assert (ur[f, n:] == SENT).all() and (dp[f, n:] == SENT).all(), f
    if n_frames > 2:
        assert ur[2, 5] == -1 and dp[2, 9] == -1 and want[2][2] == abi.ORBFE_ERR_UNSUPPORTED


def test_stereo_batch_straight_from_extraction(ex, dev):
    """The slabs orbfe_extract_batch_device writes go into the RGB-D call as they are; the host
    form on the downloaded keypoints gives the same floats."""
    import torch
    from orbslam_mapsave_amd.synth import synthetic_frame
    w, h, n = 640, 480, 2
    imgs = np.stack([synthetic_frame(40 + f, w, h) for f in range(n)])
    r = np.random.default_rng(9)
    depth = r.integers(300, 30000, (n, h, w)).astype(np.uint16)
    depth[r.random(depth.shape) < 0.1] = 0
    cap = ex.capacity(w, h)
    d_img, d_depth = up(imgs, dev), up(depth, dev)
    d_k = torch.zeros((n, cap * 28), dtype=torch.uint8, device=dev)
    d_d = torch.zeros((n, cap, 32), dtype=torch.uint8, device=dev)
    d_n = torch.zeros(n, dtype=torch.int32, device=dev)
    d_ur = torch.full((n, cap), float(SENT), dtype=torch.float32, device=dev)
    d_dp = torch.full((n, cap), float(SENT), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    ex.extract_batch_device(d_img.data_ptr(), n, w, h, w, w * h, d_k.data_ptr(), cap, d_d.data_ptr(),
                            d_n.data_ptr())
    ex.compute_stereo_from_rgbd_device(n, d_depth.data_ptr(), native.DEPTH_U16, w, h, 2 * w, 2 * w * h,
                                       float(R.FACTOR_5000), d_k.data_ptr(), d_n.data_ptr(), cap,
                                       float(R.BF), d_ur.data_ptr(), d_dp.data_ptr())
    ex.rgbd_status()
    cnt = d_n.cpu().numpy()
    keys = d_k.cpu().numpy().view(abi.KEYPOINT_DTYPE).reshape(n, cap)
    ur, dp = d_ur.cpu().numpy(), d_dp.cpu().numpy()
    for f in range(n):
        m = int(cnt[f])
        assert m > 500
        hu, hd = ex.ComputeStereoFromRGBD(depth[f], float(R.FACTOR_5000), keys[f, :m], float(R.BF))
        wu, wd, st = R.restated_stereo(depth[f], R.FACTOR_5000, keys[f, :m], None, R.BF)
        assert st == abi.ORBFE_OK and (wd > 0).sum() > 300
        assert bits(ur[f, :m]) == bits(hu) == bits(wu) and bits(dp[f, :m]) == bits(hd) == bits(wd)
        assert (ur[f, m:] == SENT).all()


# ---- close points --------------------------------------------------------------------------------

def close_host(matcher, c, mode, dists=True, sentinel=True):
    n = len(c["depth"])
    out = (np.full(n, -7, np.int32), np.full(n, 9, np.uint8), np.full((n, 3), SENT, F32),
           np.full(n, SENT, F32), np.full(n, SENT, F32))
    if not dists:
        out = out[:3] + (None, None)
    got = matcher.ClosePoints(mode, c["keys_un"], c["depth"], c["has_point"], CAMERA, c["pose"],
                              float(c["th"]), c["scale"] if dists else None, c["min_points"], out=out,
                              results=True)
    v = got["n_visited"]
    assert (out[0][v:] == -7).all() and (out[1][v:] == 9).all() and (out[2][v:] == SENT).all()
    assert not dists or ((out[3][v:] == SENT).all() and (out[4][v:] == SENT).all())
    return got


@pytest.mark.parametrize("mode", [R.CLOSE_SORTED, R.CLOSE_ALL])
@pytest.mark.parametrize("name", sorted(CLOSE))
def test_close_points_host_form(matcher, name, mode):
    c = CLOSE[name]
    assert_same(close_host(matcher, c, mode), R.run_close(c, mode), (name, mode))


def test_close_points_without_distances(matcher):
    c = CLOSE["octave_out"]  # the octave is not read: no error
    got = close_host(matcher, c, R.CLOSE_SORTED, dists=False)
    assert got["status"] == abi.ORBFE_OK
    assert_same(got, R.run_close(c, R.CLOSE_SORTED, dists=False), "no distances")
    got = matcher.ClosePoints(R.CLOSE_ALL, c["keys_un"], c["depth"], None, CAMERA, c["pose"],
                              float(c["th"]), c["scale"], results=True)
    want = R.run_close(dict(c, has_point=np.zeros(len(c["depth"]), np.uint8)), R.CLOSE_ALL)
    assert_same(got, want, "no has_point")


@pytest.mark.parametrize("mode", [R.CLOSE_SORTED, R.CLOSE_ALL])
def test_close_points_capacity_seam(matcher, mode):
    """8,192 depths > 0 are sorted exactly; 8,193 return ORBFE_ERR_CAPACITY and write nothing."""
    c = R.big_close_case(native.CLOSE_MAX_KEPT)
    assert int((c["depth"] > 0).sum()) == 8192
    assert_same(close_host(matcher, c, mode), R.run_close(c, mode), "8192")
    c = R.big_close_case(native.CLOSE_MAX_KEPT + 1)
    n = len(c["depth"])
    out = (np.full(n, -7, np.int32), np.full(n, 9, np.uint8), np.full((n, 3), SENT, F32),
           np.full(n, SENT, F32), np.full(n, SENT, F32))
    got = matcher.ClosePoints(mode, c["keys_un"], c["depth"], c["has_point"], CAMERA, c["pose"],
                              float(c["th"]), c["scale"], c["min_points"], out=out, results=True)
    assert got["status"] == abi.ORBFE_ERR_CAPACITY and got["n_visited"] == 0
    assert (out[0] == -7).all() and (out[1] == 9).all() and all((o == SENT).all() for o in out[2:])


@pytest.mark.parametrize("mode", [R.CLOSE_SORTED, R.CLOSE_ALL])
def test_close_points_batch_device(matcher, dev, mode):
    """Frames of unequal counts (one empty, one over capacity, one with an octave outside the
    pyramid) in one launch, a pose per frame: each frame equals the host form on it."""
    import torch
    frames = [CLOSE["n63"], CLOSE["M0_near"], R.big_close_case(native.CLOSE_MAX_KEPT + 1),
              CLOSE["c100_M130"], CLOSE["octave_out"], R._close_case([], [], 0)]
    th, mp = float(R.TH), R.MIN_POINTS
    frames = [dict(c, th=R.TH, min_points=mp) for c in frames]
    nf = len(frames)
    cap = max(len(c["depth"]) for c in frames) + 13
    slab = np.zeros((nf, cap), abi.KEYPOINT_DTYPE)
    depth = np.full((nf, cap), 1.0, F32)   # past a frame's count: would be kept if it were read
    hp = np.zeros((nf, cap), np.uint8)
    for f, c in enumerate(frames):
        n = len(c["depth"])
        slab[f, :n], depth[f, :n], hp[f, :n] = c["keys_un"], c["depth"], c["has_point"]
    cnt = np.asarray([len(c["depth"]) for c in frames], np.int32)
    d_k, d_z, d_hp, d_n = up(slab, dev), up(depth, dev), up(hp, dev), up(cnt, dev)
    d_pose = up(np.stack([c["pose"] for c in frames]), dev)
    d_order = torch.full((nf, cap), -7, dtype=torch.int32, device=dev)
    d_create = torch.full((nf, cap), 9, dtype=torch.uint8, device=dev)
    d_xyz = torch.full((nf, cap, 3), float(SENT), dtype=torch.float32, device=dev)
    d_mx = torch.full((nf, cap), float(SENT), dtype=torch.float32, device=dev)
    d_mn = torch.full((nf, cap), float(SENT), dtype=torch.float32, device=dev)
    d_cnt = torch.full((4, nf), -7, dtype=torch.int32, device=dev)  # visited, total, map, status
    torch.cuda.synchronize()
    p = [d_cnt[i].data_ptr() for i in range(4)]
    matcher.close_points_batch_device(mode, nf, d_k.data_ptr(), d_z.data_ptr(), d_hp.data_ptr(),
                                      d_n.data_ptr(), cap, CAMERA, d_pose.data_ptr(), th, mp, R.SCALE,
                                      d_order.data_ptr(), p[0], d_create.data_ptr(), d_xyz.data_ptr(),
                                      d_mx.data_ptr(), d_mn.data_ptr(), p[1], p[2], p[3])
    torch.cuda.synchronize()
    res = d_cnt.cpu().numpy()
    order, create, xyz = d_order.cpu().numpy(), d_create.cpu().numpy(), d_xyz.cpu().numpy()
    mx, mn = d_mx.cpu().numpy(), d_mn.cpu().numpy()
    for f, c in enumerate(frames):
        if f == 2:
            assert res[3, f] == abi.ORBFE_ERR_CAPACITY and (res[:3, f] == -7).all()
            assert (order[f] == -7).all() and (xyz[f] == SENT).all()
            continue
        if len(c["depth"]) == 0:
            assert list(res[:, f]) == [0, 0, 0, 0] and (order[f] == -7).all()
            continue
        want = close_host(matcher, c, mode)
        assert_same(want, R.run_close(c, mode), (f, "host"))
        v = int(res[0, f])
        got = {"order": order[f, :v], "create": create[f, :v], "xyz": xyz[f, :v], "max_dist": mx[f, :v],
               "min_dist": mn[f, :v], "n_visited": v, "n_total": int(res[1, f]), "n_map": int(res[2, f]),
               "status": int(res[3, f])}
        assert_same(got, want, (f, "batch"))
        assert (order[f, v:] == -7).all() and (create[f, v:] == 9).all() and (mx[f, v:] == SENT).all()
