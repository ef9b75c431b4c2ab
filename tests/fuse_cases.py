"""ORBmatcher::Fuse (ORBmatcher.cc:828-978 and 980-1103): the seeded scenario, a pure-Python
restatement of the search (everything up to bestIdx / bestDist) and a model of the map state the
loop's tail mutates, shared by the CPU and GPU tests.

The restatement follows the oracle's float reading (orb_oracle.cpp `rigid`, `camera_center`,
is_in_frustum) with Fuse's own differences: x = pc.x * invz before fx * x + cx,
KeyFrame::IsInImage's strict upper bounds, the viewing-angle test as dot < 0.5 * dist3D in
double, KeyFrame::GetFeaturesInArea without a level filter, the [lvl - 1, lvl] octave window and
the chi-square tests of the SE3 overload.
"""
from __future__ import annotations

import math

import numpy as np

import oracle
import scenarios as S

F32 = np.float32
SE3, SIM3 = 0, 1
TH_LOW = 50
LOG_SCALE = float(np.log(np.float32(1.2)).astype(np.float32))
SCALE = np.float32(1.2) ** np.arange(8, dtype=np.float32)


def inv_sigma2():
    return oracle.tables(oracle.params(1000, 1.2, 8, 32, 7))["inv_sigma2"]


def fuse_case(seed: int = 0, stereo: bool = True, kf=None, skip_rate: float = 0.1):
    """Target keyframe = extract_frame(seed, u_right); points from the frame shifted by one
    column, at depth U[2, 8] along their rays, mfMaxDistance = 0.97 dist scale[octave] (the
    predicted level stays inside the pyramid), normal = unit ray + N(0, 0.5) renormalised,
    descriptors with 6 % of the bits flipped; 300 clutter points (frustum_case's ranges, random
    normals and descriptors); all shuffled, 10 % skipped."""
    rng = np.random.Generator(np.random.PCG64(seed + 31))
    if kf is None:
        kf = S.extract_frame(seed, 1000, u_right=stereo)
    src = S.extract_frame(seed, 1000, shift=(0, 1))
    n = src.n
    z = rng.uniform(2.0, 8.0, n)
    xyz = np.stack([(src.keys["x"] - S.CX) / S.FX * z, (src.keys["y"] - S.CY) / S.FY * z, z], 1)
    dist = np.linalg.norm(xyz, axis=1)
    maxd = 0.97 * dist * SCALE[src.keys["octave"]]
    normal = xyz / dist[:, None] + rng.normal(0, 0.5, (n, 3))
    normal /= np.linalg.norm(normal, axis=1, keepdims=True)
    desc = S.flip_bits(src.desc, rng, 0.06)
    nc = 300
    cxyz = np.stack([rng.uniform(-6, 6, nc), rng.uniform(-5, 5, nc), rng.uniform(-2, 12, nc)], 1)
    cn = rng.normal(size=(nc, 3))
    cn /= np.linalg.norm(cn, axis=1, keepdims=True)
    xyz = np.concatenate([xyz, cxyz])
    normal = np.concatenate([normal, cn])
    maxd = np.concatenate([maxd, rng.uniform(2, 15, nc)])
    desc = np.concatenate([desc, S.random_desc(rng, nc)])
    perm = rng.permutation(n + nc)
    maxd = maxd[perm].astype(F32)
    return dict(kf=kf, tcw=S.pose(rng, 0.001, 0.004), cam=S.camera(bf=40.0),
                log_scale=LOG_SCALE, inv_sigma2=inv_sigma2(),
                xyz=np.ascontiguousarray(xyz[perm], F32),
                normal=np.ascontiguousarray(normal[perm], F32),
                min_dist=(maxd / SCALE[7]).astype(F32), max_dist=maxd,
                desc=np.ascontiguousarray(desc[perm]),
                skip=(rng.uniform(size=n + nc) < skip_rate).astype(np.uint8))


def subset(c: dict, idx) -> dict:
    """The case restricted to the points idx (any index expression)."""
    out = dict(c)
    for k in ("xyz", "normal", "min_dist", "max_dist", "desc", "skip"):
        out[k] = np.ascontiguousarray(c[k][idx])
    return out


def camera_center(T):
    return [F32(-(float(T[0, i]) * float(T[0, 3]) + float(T[1, i]) * float(T[1, 3]) +
                  float(T[2, i]) * float(T[2, 3]))) for i in range(3)]


# Single-decision mutants of the gates (tests/projection_cases.py builds the inputs that show
# them): the first four change project(), the others search_point().
GATE_MUTANTS = ("bounds_inclusive_upper", "vcos_float_quotient", "chi2_float_literal",
                "chi2_mono_uses_78", "stereo_kr_gt0", "sigma_of_predicted_level", "window_plus1",
                "sim3_has_chi2")
# `z <= 0` is no mutant: z = +-0 makes invz infinite and u, v NaN or infinite, which
# KeyFrame::IsInImage refuses (a NaN fails `x >= mnMinX`), so the point is dropped either way.
# chi2_float_literal shows at 7.8 only ((float)7.8 > 7.8 > its predecessor); (float)5.99 lies
# below 5.99 and no float lies between them.  The chi-square mutants show in the SE3 mode,
# sim3_has_chi2 in the Sim3 mode.
GATE_EQUIVALENT = ("depth_le0",)
SE3_ONLY = ("chi2_float_literal", "chi2_mono_uses_78", "stereo_kr_gt0", "sigma_of_predicted_level")


def project(c: dict, i: int, ow=None, mutant=None):
    """The projection block of both overloads for point i -> dict(pc, u, v, ur, dist, dot,
    reject) with reject in (None, "depth", "image", "distance", "angle") and, when not rejected,
    lvl (MapPoint::PredictScale, unclamped; None where log(ratio) / logScaleFactor is not
    finite and its conversion to int undefined)."""
    kf, cam = c["kf"], c["cam"]
    T = c["tcw"].astype(F32)
    if ow is None:
        ow = camera_center(T)
    P = c["xyz"][i]
    pc = [((T[r, 0] * P[0] + T[r, 1] * P[1]) + T[r, 2] * P[2]) + T[r, 3] for r in range(3)]
    out = dict(pc=pc, reject=None)
    if (pc[2] <= F32(0.0)) if mutant == "depth_le0" else (pc[2] < F32(0.0)):
        out["reject"] = "depth"
        return out
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        invz = F32(1.0) / pc[2]
        x, y = pc[0] * invz, pc[1] * invz
        u = F32(cam.fx) * x + F32(cam.cx)
        v = F32(cam.fy) * y + F32(cam.cy)
        ur = u - F32(cam.bf) * invz
    out.update(u=u, v=v, ur=ur)
    if mutant == "bounds_inclusive_upper":
        inside = u >= F32(kf.min_x) and u <= F32(kf.max_x) and v >= F32(kf.min_y) and \
            v <= F32(kf.max_y)
    else:                                           # KeyFrame::IsInImage: a NaN is outside
        inside = u >= F32(kf.min_x) and u < F32(kf.max_x) and v >= F32(kf.min_y) and \
            v < F32(kf.max_y)
    if not inside:
        out["reject"] = "image"
        return out
    po = [P[j] - ow[j] for j in range(3)]
    d3 = F32(math.sqrt(float(po[0]) * float(po[0]) + float(po[1]) * float(po[1]) +
                       float(po[2]) * float(po[2])))
    out["dist"] = d3
    if d3 < F32(0.8) * c["min_dist"][i] or d3 > F32(1.2) * c["max_dist"][i]:
        out["reject"] = "distance"
        return out
    nv = c["normal"][i]
    dot = float(po[0]) * float(nv[0]) + float(po[1]) * float(nv[1]) + float(po[2]) * float(nv[2])
    out["dot"] = dot
    if mutant == "vcos_float_quotient":             # isInFrustum's form of the test
        with np.errstate(all="ignore"):
            steep = F32(np.float64(dot) / np.float64(d3)) < F32(0.5)
    else:
        steep = dot < 0.5 * float(d3)
    if steep:
        out["reject"] = "angle"
        return out
    with np.errstate(all="ignore"):
        ratio = c["max_dist"][i] / d3
        lg = math.log(float(ratio)) if 0 < ratio < np.inf else \
            (np.inf if ratio > 0 else -np.inf if ratio == 0 else np.nan)
        q = F32(lg) / F32(c["log_scale"])
    out["lvl"] = int(math.ceil(float(q))) if np.isfinite(q) else None
    return out


def search_point(c: dict, i: int, th: float, mode: int, ow=None, stats=None, mutant=None):
    """(best_idx, best_dist, unsupported) of point i, the skip byte not looked at."""
    kf = c["kf"]
    p = project(c, i, ow, mutant)
    if p["reject"] is not None:
        if stats is not None:
            stats[p["reject"]] = stats.get(p["reject"], 0) + 1
        return -1, 256, False
    lvl = p["lvl"]
    if lvl is None or lvl < 0 or lvl >= len(kf.scale_factors):
        if stats is not None:
            stats["level_outside"] = stats.get("level_outside", 0) + 1
        return -1, 256, True
    u, v, ur = p["u"], p["v"], p["ur"]
    r = F32(th) * kf.scale_factors[lvl]
    k = kf.keys
    best, bi = 256, -1
    for idx in oracle.features_in_area(kf, float(u), float(v), float(r)):
        octave = int(k["octave"][idx])
        if octave < lvl - 1 or octave > (lvl + 1 if mutant == "window_plus1" else lvl):
            if stats is not None:
                stats["level_window"] = stats.get("level_window", 0) + 1
            continue
        if mode == SE3 or mutant == "sim3_has_chi2":
            ex, ey = u - k["x"][idx], v - k["y"][idx]
            inv = c["inv_sigma2"][lvl if mutant == "sigma_of_predicted_level" else octave]
            kr = kf.u_right[idx] if kf.u_right is not None else F32(-1)
            # the float product against the double literals 7.8 / 5.99 (928, 939)
            if (kr > 0) if mutant == "stereo_kr_gt0" else (kr >= 0):
                er = ur - kr
                e2 = ex * ex + ey * ey + er * er
                drop = e2 * inv > F32(7.8) if mutant == "chi2_float_literal" else \
                    float(e2 * inv) > 7.8
                if stats is not None:
                    stats["chi2_stereo"] = stats.get("chi2_stereo", 0) + 1
            else:
                e2 = ex * ex + ey * ey
                if mutant == "chi2_float_literal":
                    drop = e2 * inv > F32(5.99)
                else:
                    drop = float(e2 * inv) > (7.8 if mutant == "chi2_mono_uses_78" else 5.99)
                if stats is not None:
                    stats["chi2_mono"] = stats.get("chi2_mono", 0) + 1
            if drop:
                if stats is not None:
                    stats["chi2"] = stats.get("chi2", 0) + 1
                continue
        d = int(np.unpackbits(c["desc"][i] ^ kf.desc[idx]).sum())
        if d < best:
            best, bi = d, int(idx)
    return (bi if best <= TH_LOW else -1), best, False


def restated(c: dict, th: float, mode: int, use_skip: bool = True, stats=None, mutant=None):
    """-> (best_idx, best_dist, n_found, unsupported) for every point of the case."""
    n = len(c["xyz"])
    ow = camera_center(c["tcw"].astype(F32))
    bi = np.full(n, -1, np.int32)
    bd = np.full(n, 256, np.int32)
    bad = False
    for i in range(n):
        if use_skip and c["skip"][i]:
            if stats is not None:
                stats["skip"] = stats.get("skip", 0) + 1
            continue
        bi[i], bd[i], u = search_point(c, i, th, mode, ow, stats, mutant)
        bad |= u
    return bi, bd, int((bi >= 0).sum()), bad


# ---- the map state the tail of the loop mutates -----------------------------------------------

class MapModel:
    """One keyframe's slots and the points' mutable state.  Point ids: the list entries to fuse
    refer to ids 0 .. n_pts - 1 through `pid` (an id may appear twice in the list), the points the
    keyframe already holds have ids from n_pts up."""

    def __init__(self, n_kp: int, pid: np.ndarray, seed: int):
        rng = np.random.Generator(np.random.PCG64(seed + 97))
        self.pid = np.asarray(pid, np.int64)
        n_pts = int(self.pid.max()) + 1 if len(self.pid) else 0
        held = rng.uniform(size=n_kp) < 0.5          # slots that hold a point
        self.slot = np.where(held, n_pts + np.arange(n_kp), -1).astype(np.int64)
        total = n_pts + n_kp
        self.nobs = rng.integers(1, 6, total)
        self.bad = np.zeros(total, bool)
        self.bad[:n_pts] = rng.uniform(size=n_pts) < 0.05
        self.bad[n_pts:] = rng.uniform(size=n_kp) < 0.1   # pMPinKF->isBad()
        self.in_kf = np.zeros(total, bool)
        self.in_kf[n_pts:] = held
        # a few of the points to fuse sit in the keyframe already (IsInKeyFrame / spAlreadyFound)
        free = np.flatnonzero(~held)
        take = rng.choice(n_pts, size=min(n_pts // 20, len(free)), replace=False)
        for p, s in zip(take, rng.choice(free, size=len(take), replace=False)):
            self.slot[s] = p
            self.in_kf[p] = True
        self.replaced = []   # SE3: (bad point, its replacement); Sim3: (list entry, pMPinKF)
        self.added = []      # (point, keypoint)
        self.calls = []      # the walk's call sequence: ("O" | "E", list entry, keypoint)

    def skipped(self, i: int) -> bool:
        p = self.pid[i]
        return bool(self.bad[p] or self.in_kf[p])

    def static_skip(self) -> np.ndarray:
        return np.array([self.skipped(i) for i in range(len(self.pid))], np.uint8)

    def _replace(self, old: int, new: int):
        """MapPoint::Replace (MapPoint.cc:358-397) within this keyframe."""
        self.bad[old] = True
        s = np.flatnonzero(self.slot == old)
        if len(s):
            if not self.in_kf[new]:
                self.slot[s[0]] = new
                self.in_kf[new] = True
            else:
                self.slot[s[0]] = -1
            self.in_kf[old] = False
        self.nobs[new] += self.nobs[old]
        self.replaced.append((int(old), int(new)))

    def apply(self, i: int, idx: int, mode: int):
        """Lines 955-974 (SE3) / 1085-1099 (Sim3) for list entry i and keypoint idx."""
        p = self.pid[i]
        pin = self.slot[idx]
        if pin >= 0:
            self.calls.append(("O", int(i), int(idx)))
            if not self.bad[pin]:
                if mode == SIM3:
                    self.replaced.append((int(i), int(pin)))
                elif self.nobs[pin] > self.nobs[p]:
                    self._replace(p, pin)
                else:
                    self._replace(pin, p)
        else:
            self.calls.append(("E", int(i), int(idx)))
            self.nobs[p] += 1
            self.in_kf[p] = True
            self.slot[idx] = p
            self.added.append((int(p), int(idx)))

    def result(self):
        return self.slot.tolist(), self.replaced, self.added, self.bad.tolist()


def sequential(model: MapModel, search, mode: int) -> int:
    """The reference loop: skip test, search and apply interleaved.  search(i) -> best_idx."""
    n = 0
    for i in range(len(model.pid)):
        if model.skipped(i):
            continue
        idx = search(i)
        if idx >= 0:
            model.apply(i, idx, mode)
            n += 1
    return n


def walk(model: MapModel, best_idx, mode: int) -> int:
    """The decomposed form: best_idx from one batched search, then the ordered walk with the
    skip test re-evaluated against live state."""
    n = 0
    for i in range(len(model.pid)):
        if model.skipped(i):
            continue
        if best_idx[i] >= 0:
            model.apply(i, int(best_idx[i]), mode)
            n += 1
    return n


def sim3_normalise(scw: np.ndarray) -> np.ndarray:
    """ORBmatcher.cc:989-992 as the C++ adapter reads it: scw = (float)sqrt of the double dot
    product of row 0 of sRcw, then every entry times the float (float)(1.0 / scw)."""
    s = scw.astype(F32).reshape(3, 4)
    n = F32(math.sqrt(sum(float(x) * float(x) for x in s[0, :3])))
    return (s * F32(1.0 / float(n))).astype(F32)


def dump_case(path: str, c: dict, model: MapModel, th_se3: float, th_sim3: float,
              scw: np.ndarray):
    """The case file tests/cpp/fuse_test.cpp reads."""
    kf = c["kf"]
    cam = c["cam"]
    n_ids = len(model.nobs)
    with open(path, "wb") as f:
        np.array([kf.n, kf.u_right is not None, len(c["xyz"]), len(kf.scale_factors), n_ids],
                 np.int32).tofile(f)
        np.array([kf.min_x, kf.max_x, kf.min_y, kf.max_y, cam.fx, cam.fy, cam.cx, cam.cy, cam.bf,
                  cam.b, c["log_scale"], th_se3, th_sim3], F32).tofile(f)
        c["tcw"].astype(F32).tofile(f)
        scw.astype(F32).tofile(f)
        kf.scale_factors.tofile(f)
        c["inv_sigma2"][:len(kf.scale_factors)].astype(F32).tofile(f)
        kf.keys.tofile(f)
        kf.desc.tofile(f)
        (kf.u_right if kf.u_right is not None else np.full(kf.n, -1, F32)).tofile(f)
        for k in ("xyz", "normal", "min_dist", "max_dist", "desc"):
            c[k].tofile(f)
        model.pid.astype(np.int32).tofile(f)
        model.slot.astype(np.int32).tofile(f)
        model.nobs.astype(np.int32).tofile(f)
        model.bad.astype(np.uint8).tofile(f)
        model.in_kf.astype(np.uint8).tofile(f)


def walk_case(seed: int, n_take: int = 400):
    """A list of points to fuse with repeated entries (the second occurrence must be skipped
    once the first was added or replaced) over fuse_case(seed)."""
    c = fuse_case(seed)
    rng = np.random.Generator(np.random.PCG64(seed + 131))
    n = len(c["xyz"])
    first = rng.choice(n, size=min(n_take, n), replace=False)
    dup = rng.choice(first, size=len(first) // 8, replace=False)
    order = np.concatenate([first, dup])
    order = order[rng.permutation(len(order))]
    # pid: list entry -> point id (entries sharing a point share an id)
    _, pid = np.unique(order, return_inverse=True)
    return subset(c, order), pid
