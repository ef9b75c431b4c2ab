"""MapPoint::UpdateNormalAndDepth (MapPoint.cc:571-619), ComputeDistinctiveDescriptors (:483-548),
the mpRefKF rule of EraseObservation (:367-368) and the map-point loop of
LocalMapping::ProcessNewKeyFrame (LocalMapping.cc:140-161) restated in plain Python over the
scripted map model of tests/culling_cases.py: real per-point dicts walked in key order, numpy
float32 / float64 for the arithmetic, branch counters and single-decision mutants; the built cases
that tests/test_refresh.py proves non-trivial and tests/test_gpu_refresh.py runs against the
library; and the driver that replays a script on a ``native.LocalMap``.

The script operations of culling_cases are kept.  New:
    ("scale", [factors])                         mvScaleFactors of the map
    ("centers", [kfs], [[x, y, z], ...])         GetCameraCenter()
    ("descs", kf, uint8 array (slots, 32))       mDescriptors
    ("refkf", [points], [kf | None, ...])        mpRefKF, plain assignment
    ("xyz", [points], [[x, y, z], ...])          mWorldPos (the caller's array)
    ("refresh", what, [point | None | OOB, ...]) both functions by the bits of `what`, over a list
                                                 -> the per-entry masks, or ("unsupported", masks)
    ("refreshkf", kf, what)                      the same over the keyframe's mvpMapPoints
                                                 -> the number of entries that hold a live point
    ("process", kf[, recent_cap])                the loop of ProcessNewKeyFrame -> recent
The answer of each of the last three is its own output and the whole state: culling_cases' state,
every point's mpRefKF and its normal, distances and descriptor as bit patterns (a NaN as "nan");
a refusal answers ("error", state) or ("capacity", state) with nothing changed.
"""
from __future__ import annotations

import random

import numpy as np

import culling_cases as Q
from culling_cases import Capacity, Refused
from localmap_cases import BASE, MP, _bump, keys_for

MUTANTS = ("tie_slot_order", "sum_slot_order", "float_norm", "divide", "recip_double", "fma",
           "desc_counts_bad", "normal_skips_bad", "normal_on_null_ref", "missing_ref_last",
           "min_scale_level", "median_half", "tie_last", "ref_lowest_slot", "ref_after_bad",
           "ref_kept_when_bad", "recent_first", "process_right_ignored")

ND, DESC, UNSUP = 1, 2, 4          # ORBFE_MAP_REFRESH_*
MAX_OBS = 1024                     # ORBFE_MAP_MAX_REFRESH_OBS
OOB = "<outside the map>"          # a list entry that is no point slot
F32 = np.float32

# what no refresh has written yet: the caller's arrays start at these
SENT_NORMAL, SENT_MIN, SENT_MAX, SENT_DESC = 1234.5, -7.0, -9.0, 0xA5


def _fbits(a):
    a = np.asarray(a, F32).reshape(-1)
    return tuple("nan" if np.isnan(x) else int(b) for x, b in zip(a, a.view(np.uint32)))


_POP = np.array([bin(i).count("1") for i in range(256)], np.int64)


def hamming_row(v, i):
    """ORBmatcher::DescriptorDistance of descriptor i to every descriptor of v."""
    return [int(x) for x in _POP[np.bitwise_xor(v, v[i])].sum(1)]


# ---- the three readings of cv::Mat arithmetic, one helper each
def recip(s, mutant=None):
    """Mat / double: the scale 1 / s taken as a float."""
    r = 1.0 / np.float64(s)
    return r if mutant == "recip_double" else F32(r)


def axpy(acc, d, a, mutant=None):
    """Mat + Mat * a: the product rounded to float, then the sum."""
    if mutant == "fma":
        return F32(np.float64(d) * np.float64(a) + np.float64(acc))
    return F32(acc + F32(d * a))


def mean(acc, n):
    """Mat / int: the scale 1 / n taken as a float."""
    return F32(acc * F32(1.0 / np.float64(n)))


def norm(d, mutant=None):
    """cv::norm of a 3x1 CV_32F: squares summed in double, index order (H25)."""
    if mutant == "float_norm":
        return np.sqrt(F32(F32(F32(d[0] * d[0]) + F32(d[1] * d[1])) + F32(d[2] * d[2])))
    return np.sqrt((np.float64(d[0]) * d[0] + np.float64(d[1]) * d[1]) + np.float64(d[2]) * d[2])


class ObsMap(dict):
    """mObservations of one point; an erase runs MapPoint.cc:367-368."""

    def __init__(self, owner, items=()):
        super().__init__(items)
        self.owner = owner

    def __delitem__(self, kf):
        super().__delitem__(kf)
        self.owner.model.on_erase(self.owner, kf)


class _MP(MP):
    """A point whose `obs` stays an ObsMap whatever is assigned to it (SetBadFlag assigns {})."""

    @property
    def obs(self):
        return self.__dict__["_obs"]

    @obs.setter
    def obs(self, v):
        self.__dict__["_obs"] = ObsMap(self, v)


def _wrap_point(mp, model):
    old = mp.__dict__.pop("obs", {})
    mp.__class__ = _MP
    mp.model = model
    mp.obs = old


class Model(Q.Model):
    """culling_cases.Model plus, per map: scale; per keyframe: center, desc (None: never set); per
    point: ref, pos and the caller's four arrays normal, mind, maxd, desc."""

    def clear(self):
        super().clear()
        self.scale = None
        self.mutant = None
        self.st = None
        self.plain_erase = False

    def apply(self, op):
        k = op[0]
        if k == "points":
            super().apply(op)
            for n in op[1]:
                mp = self.mps[n]
                _wrap_point(mp, self)
                mp.ref = None
                mp.pos = np.zeros(3, F32)
                mp.normal = np.full(3, SENT_NORMAL, F32)
                mp.mind, mp.maxd = F32(SENT_MIN), F32(SENT_MAX)
                mp.desc = np.full(32, SENT_DESC, np.uint8)
        elif k == "kf":
            super().apply(op)
            self.kfs[op[1]].center = np.zeros(3, F32)
            self.kfs[op[1]].desc = None
        elif k == "scale":
            if not 1 <= len(op[1]) <= 128:
                raise Refused("nlevels")
            self.scale = [F32(x) for x in op[1]]
        elif k == "centers":
            for n, c in zip(op[1], op[2]):
                self.kfs[n].center = np.asarray(c, F32).copy()
        elif k == "descs":
            d = np.asarray(op[2], np.uint8).reshape(-1, 32)
            if len(d) != len(self.kfs[op[1]].mps):
                raise Refused("one row per slot")
            self.kfs[op[1]].desc = d.copy()
        elif k == "refkf":
            for p, f in zip(op[1], op[2]):
                self.mps[p].ref = f
        elif k == "xyz":
            for p, x in zip(op[1], op[2]):
                self.mps[p].pos = np.asarray(x, F32).copy()
        else:
            super().apply(op)

    def erase_plain(self, p, kf):
        self.plain_erase = True
        try:
            super().erase_plain(p, kf)
        finally:
            self.plain_erase = False

    # ---- MapPoint.cc:367-368, called by every `del mp.obs[kf]` of the model
    def on_erase(self, mp, kf):
        m, st = self.mutant, self.st
        if mp.ref != kf:                                                   # :367
            _bump(st, "erase_ref_other")
            return
        will_bad = not self.plain_erase and mp.nobs <= 2                   # what :371 decides next
        if will_bad and m == "ref_kept_when_bad":
            return
        if not mp.obs or (will_bad and m == "ref_after_bad"):
            _bump(st, "erase_ref_empty")
            mp.ref = None                                                  # begin() of an empty map: H29
            return
        _bump(st, "erase_ref_bad" if will_bad else "erase_ref_next")
        by = (lambda f: self.kfs[f].slot) if m == "ref_lowest_slot" else (lambda f: self.kfs[f].key)
        first = min(mp.obs, key=by)                                        # :368, begin()->first
        if first != min(mp.obs, key=lambda f: self.kfs[f].slot):
            _bump(st, "erase_ref_key_not_slot")
        mp.ref = first

    def _ordered(self, mp, by_slot):
        key = (lambda e: self.kfs[e[0]].slot) if by_slot else (lambda e: self.kfs[e[0]].key)
        return sorted(mp.obs.items(), key=key)                             # map<KeyFrame*, size_t>

    # ---- MapPoint.cc:483-548
    def distinctive(self, p, mutant=None, st=None):
        mp = self.mps[p]
        if mp.bad:                                                         # :492
            _bump(st, "dd_bad")
            return False
        obs = self._ordered(mp, mutant == "tie_slot_order")
        if not obs:                                                        # :497
            _bump(st, "dd_empty")
            return False
        v = []
        for f, idx in obs:                                                 # :502
            kf = self.kfs[f]
            if not kf.bad or mutant == "desc_counts_bad":                  # :506
                v.append(kf.desc[idx])
            else:
                _bump(st, "dd_bad_observer")
        if not v:                                                          # :510
            _bump(st, "dd_all_bad")
            return False
        N = len(v)
        v = np.stack(v)
        dist = [hamming_row(v, i) for i in range(N)]                       # :516-526
        best_median, best = 1 << 31, 0                                     # :529-530
        for i in range(N):
            vd = sorted(dist[i])
            median = vd[N // 2 if mutant == "median_half" else int(0.5 * (N - 1))]  # :535
            if median == best_median:
                _bump(st, "dd_tie")
            if median < best_median or (mutant == "tie_last" and median <= best_median):  # :537
                best_median, best = median, i
        _bump(st, "dd_written")
        mp.desc = v[best].copy()                                           # :546
        return True

    # ---- MapPoint.cc:571-619
    def _ref_level(self, mp, mutant=None):
        """(level, supported) of `pRefKF->mvKeysUn[observations[pRefKF]].octave`."""
        kf = self.kfs[mp.ref]
        idx = mp.obs.get(mp.ref, -1 if mutant == "missing_ref_last" else 0)  # operator[]: 0
        if idx is None or not -len(kf.mps) <= idx < len(kf.mps):
            return 0, False                                                # no keypoint to read
        level = kf.octave[idx]
        return level, level < len(self.scale)

    def normal_depth(self, p, mutant=None, st=None):
        """-> 0 (nothing written), ND, or UNSUP."""
        mp = self.mps[p]
        if mp.bad:                                                         # :579
            _bump(st, "nd_bad")
            return 0
        obs = self._ordered(mp, mutant == "sum_slot_order")
        if not obs:                                                        # :586
            _bump(st, "nd_empty")
            return 0
        with np.errstate(all="ignore"):
            acc = [F32(0), F32(0), F32(0)]
            n = 0
            for f, _ in obs:                                               # :591
                if self.kfs[f].bad:
                    _bump(st, "nd_bad_observer")
                    if mutant == "normal_skips_bad":
                        continue
                d = mp.pos - self.kfs[f].center                            # :595
                nrm = norm(d, mutant)
                if mutant == "divide":
                    acc = [F32(acc[k] + F32(d[k] / F32(nrm))) for k in range(3)]
                else:
                    a = recip(nrm, mutant)
                    acc = [axpy(acc[k], d[k], a, mutant) for k in range(3)]  # :596
                n += 1
            if mp.ref is None:                                             # :600
                _bump(st, "nd_null_ref")
                if mutant == "normal_on_null_ref":
                    mp.normal = np.array([mean(a, n) for a in acc], F32)
                return 0
            _bump(st, "nd_ref_observer" if mp.ref in mp.obs else "nd_ref_absent")
            if self.kfs[mp.ref].bad:
                _bump(st, "nd_ref_bad")
            level, ok = self._ref_level(mp, mutant)
            if not ok:
                _bump(st, "nd_unsupported")
                return UNSUP
            dist = F32(norm(mp.pos - self.kfs[mp.ref].center))             # :606-607
            mp.maxd = F32(dist * self.scale[level])                        # :615
            top = self.scale[level if mutant == "min_scale_level" else len(self.scale) - 1]
            mp.mind = F32(mp.maxd / top)                                   # :616
            mp.normal = np.array([mean(a, n) for a in acc], F32)           # :617
        _bump(st, "nd_written")
        return ND

    def _refresh_check(self, names, what, extra=0):
        """What the check launch finds before anything is written (`extra`: observers each listed
        point is about to gain)."""
        if what & ND and self.scale is None:
            raise Refused("no scale table")
        arg = cap = False
        for p in names:
            if p is None:
                continue
            if p == OOB:
                arg = True
                continue
            mp = self.mps[p]
            if mp.bad:
                continue
            if len(mp.obs) + extra > MAX_OBS:
                cap = True
                continue
            for f, idx in mp.obs.items():
                if idx is None:
                    arg = True
                elif what & DESC and not self.kfs[f].bad and self.kfs[f].desc is None:
                    arg = True
        if arg:
            raise Refused("refresh")
        if cap:
            raise Capacity("observers")

    def refresh(self, names, what, mutant=None, st=None):
        self._refresh_check(names, what)
        masks = []
        for p in names:
            if p is None:
                _bump(st, "list_null")
                masks.append(0)
                continue
            if p in names[:len(masks)]:
                _bump(st, "list_repeat")
            m = 0
            if what & ND:
                m |= self.normal_depth(p, mutant, st)
            if what & DESC and self.distinctive(p, mutant, st):
                m |= DESC
            masks.append(m)
        return ("unsupported", masks) if any(m & UNSUP for m in masks) else masks

    # ---- LocalMapping.cc:140-161
    def process(self, name, cap, mutant=None, st=None):
        kf = self.kfs[name]
        if self.scale is None:
            raise Refused("no scale table")
        plan, seen = [], set()
        for i, p in enumerate(kf.mps):                                     # :142
            if p is None:                                                  # :145
                _bump(st, "pk_null")
                continue
            mp = self.mps[p]
            if mp.bad:                                                     # :147
                _bump(st, "pk_bad")
                continue
            if name in mp.obs or p in seen:                                # :149
                _bump(st, "pk_second_index" if p in seen else "pk_observed")
                plan.append(("recent", p, i))
            elif mutant == "recent_first" and p in kf.mps[i + 1:]:
                plan.append(("recent", p, i))
            else:
                seen.add(p)
                plan.append(("add", p, i))
        recent = [p for what, p, _ in plan if what == "recent"]
        if len(recent) > cap:
            raise Capacity(len(recent))
        adds = [p for what, p, _ in plan if what == "add"]
        if adds and kf.desc is None:
            raise Refused("the new observer has no descriptors")
        self._refresh_check(adds, ND | DESC, 1)
        for what, p, i in plan:
            if what != "add":
                continue
            self.add_observation(p, name, i, "right_ignored" if mutant == "process_right_ignored" else mutant, st)  # :151
            self.normal_depth(p, mutant, st)                               # :152
            self.distinctive(p, mutant, st)                                # :153
        return recent                                                      # :157

    def state(self):
        refs = {n: mp.ref for n, mp in self.mps.items()}
        arrs = {n: (_fbits(mp.normal), _fbits([mp.mind, mp.maxd]), bytes(mp.desc)) for n, mp in self.mps.items()}
        return super().state() + (refs, arrs)

    def run(self, op, mutant=None, st=None):
        k = op[0]
        self.mutant, self.st = mutant, st
        out = None
        try:
            if k == "refresh":
                out = self.refresh(list(op[2]), op[1], mutant, st)
            elif k == "refreshkf":
                names = list(self.kfs[op[1]].mps)
                self.refresh(names, op[2], mutant, st)
                out = sum(1 for p in names if p is not None and not self.mps[p].bad)
            elif k == "process":
                out = self.process(op[1], op[2] if len(op) > 2 else 8192, mutant, st)
            elif k in ("scale", "centers", "descs", "refkf", "xyz"):
                self.apply(op)
                return None
            else:
                return super().run(op, mutant, st)
        except Refused:
            return "error", self.state()
        except Capacity:
            return "capacity", self.state()
        return out, self.state()


def run_script(script, mutant=None, stats=None):
    m, out = Model(), []
    for op in script:
        a = m.run(op, mutant, stats)
        if a is not None:
            out.append(a)
    return out


# ---- the driver over native.LocalMap -----------------------------------------------------------
class LibraryRunner(Q.LibraryRunner):
    """Replays a script on a ``native.LocalMap`` with the caller's map-wide arrays in device memory
    (torch); after every refresh operation the whole state is read back through the getters.
    `form`: how a refresh is issued, "host" (list uploaded), "device" (list in device memory) or
    "kf" (the keyframe form wherever the operation is a refreshkf).  `desc_via`: "host" or
    "device", how descriptors are set."""

    def __init__(self, lm, batch="batch", form="host", desc_via="host"):
        super().__init__(lm, batch)
        import torch
        self.torch, self.form, self.desc_via = torch, form, desc_via
        self.cap = 0
        self.t = {}
        self._grow(64)

    def _grow(self, n):
        if n <= self.cap:
            return
        torch, cap = self.torch, max(2 * self.cap, n)
        new = {"xyz": torch.zeros(cap, 3, dtype=torch.float32, device="cuda"),
               "normal": torch.full((cap, 3), SENT_NORMAL, dtype=torch.float32, device="cuda"),
               "min_dist": torch.full((cap,), SENT_MIN, dtype=torch.float32, device="cuda"),
               "max_dist": torch.full((cap,), SENT_MAX, dtype=torch.float32, device="cuda"),
               "desc": torch.full((cap, 32), SENT_DESC, dtype=torch.uint8, device="cuda")}
        for k, v in self.t.items():
            new[k][:self.cap] = v
        self.t, self.cap = new, cap
        torch.cuda.synchronize()    # the handle has a stream of its own

    def arrays(self):
        from orbslam_mapsave_amd.native import MapPointArrays
        return MapPointArrays(**{k: v.data_ptr() for k, v in self.t.items()})

    def state(self):
        lm, kn, pn = self.lm, self.kf_names, self.mp_names
        self.torch.cuda.synchronize()
        refs = lm.GetReferenceKeyFrame(list(range(len(pn)))) if pn else []
        nrm, mn, mx, ds = (self.t[k].cpu().numpy() for k in ("normal", "min_dist", "max_dist", "desc"))
        arrs = {n: (_fbits(nrm[i]), _fbits([mn[i], mx[i]]), bytes(ds[i])) for i, n in enumerate(pn)}
        return super().state() + ({n: None if r < 0 else kn[r] for n, r in zip(pn, refs)}, arrs)

    def _slots(self, names):
        return [-1 if p is None else len(self.mp_names) + 5 if p == OOB else self.mp[p] for p in names]

    def _refresh(self, what, slots):
        torch = self.torch
        if self.form == "host":
            return [int(x) for x in self.lm.RefreshPoints(what, slots, self.arrays())]
        d_list = torch.tensor(slots + [0], dtype=torch.int32, device="cuda")
        d_res = torch.full((len(slots) + 1,), 0xEE, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        try:
            self.lm.RefreshPoints(what, None, self.arrays(), d_list=d_list.data_ptr(), n=len(slots),
                                  d_result=d_res.data_ptr())
        except Exception as e:
            e.result = d_res.cpu().numpy()[:len(slots)]
            raise
        return [int(x) for x in d_res.cpu().numpy()[:len(slots)]]

    def apply(self, op):
        from orbslam_mapsave_amd import abi
        k, lm = op[0], self.lm
        out = None
        try:
            if k == "points":
                r = super().apply(op)
                self._grow(len(self.mp_names))
                return r
            if k == "scale":
                lm.SetScaleFactors(op[1])
                assert lm.GetScaleFactors().tobytes() == np.asarray(op[1], F32).tobytes()
                return None
            if k == "centers":
                ks = [self.kf[n] for n in op[1]]
                lm.SetCameraCenter(ks, op[2])
                assert lm.GetCameraCenter(ks).tobytes() == np.asarray(op[2], F32).tobytes()
                return None
            if k == "descs":
                d = np.ascontiguousarray(op[2], np.uint8).reshape(-1, 32)
                if self.desc_via == "device" and len(d) == len(lm.get_keyframe_points(self.kf[op[1]])):
                    t = self.torch.from_numpy(d).cuda()
                    self.torch.cuda.synchronize()
                    lm.SetDescriptors(self.kf[op[1]], d_desc=t.data_ptr(), n=len(d))
                else:
                    lm.SetDescriptors(self.kf[op[1]], d)
                got, was_set = lm.GetDescriptors(self.kf[op[1]])
                assert was_set and got.tobytes() == d.tobytes()
                return None
            if k == "refkf":
                lm.SetReferenceKeyFrame([self.mp[p] for p in op[1]], [-1 if f is None else self.kf[f] for f in op[2]])
                return None
            if k == "xyz":
                idx = self.torch.tensor([self.mp[p] for p in op[1]], dtype=self.torch.long, device="cuda")
                self.t["xyz"][idx] = self.torch.from_numpy(np.asarray(op[2], F32).reshape(-1, 3)).cuda()
                self.torch.cuda.synchronize()
                return None
            if k == "refresh":
                out = self._refresh(op[1], self._slots(op[2]))
            elif k == "refreshkf":
                s = self.kf[op[1]]
                if self.form == "kf":
                    out = lm.RefreshKeyFramePoints(s, self.arrays(), op[2])
                else:
                    row = [int(x) for x in lm.get_keyframe_points(s)]
                    live = [x for x in row if x >= 0]
                    bad = lm.get_bad_flags(1, live) if live else []
                    if row:
                        self._refresh(op[2], row)
                    elif op[2] & ND and not len(lm.GetScaleFactors()):
                        raise abi.OrbfeError("no scale table", abi.ORBFE_ERR_ARG)
                    out = int(sum(1 for b in bad if not b))
            elif k == "process":
                rec = lm.ProcessNewKeyFrame(self.kf[op[1]], self.arrays(), op[2] if len(op) > 2 else 8192)
                out = [self.mp_names[s] for s in rec]
            else:
                return super().apply(op)
        except abi.OrbfeError as e:
            if e.status == abi.ORBFE_ERR_UNSUPPORTED and k == "refresh":
                return ("unsupported", [int(x) for x in e.result]), self.state()
            if e.status == abi.ORBFE_ERR_UNSUPPORTED and k == "refreshkf":
                row = [int(x) for x in lm.get_keyframe_points(self.kf[op[1]])]
                live = [x for x in row if x >= 0]
                bad = lm.get_bad_flags(1, live) if live else []
                return int(sum(1 for b in bad if not b)), self.state()
            if e.status == abi.ORBFE_ERR_CAPACITY:
                return "capacity", self.state()
            assert e.status == abi.ORBFE_ERR_ARG, e
            return "error", self.state()
        return out, self.state()


# ---- built cases -------------------------------------------------------------------------------
SCALE8 = [float(F32(1.2) ** i) for i in range(8)]


def _desc_rows(seed, n):
    return np.random.RandomState(seed).randint(0, 256, (n, 32)).astype(np.uint8)


def _world(v, nkf, slots=6, points=None, octave=None, right_every=3, descs=True):
    """nkf keyframes of `slots` slots; point P_j is held at slot j of every keyframe and observed
    there.  Keys run against the slots (keys_for).  Centres, descriptors, features, scale set."""
    s, keys = [], keys_for(nkf, v)
    pts = [f"P{j}" for j in range(slots)] if points is None else points
    s.append(("points", pts))
    for i in range(nkf):
        s.append(("kf", f"K{i}", keys[i], pts + [None] * (slots - len(pts))))
    s.append(("scale", SCALE8))
    r = random.Random(50 + v)
    for i in range(nkf):
        s.append(("features", f"K{i}", [(octave if octave is not None else (i + j) % 8) for j in range(slots)],
                  [1.0 if (i + j) % right_every == 0 else -1.0 for j in range(slots)], None, 40.0))
        if descs:
            s.append(("descs", f"K{i}", _desc_rows(1000 * v + i, slots)))
    s.append(("centers", [f"K{i}" for i in range(nkf)],
              [[r.uniform(-3, 3), r.uniform(-3, 3), r.uniform(-3, 3)] for _ in range(nkf)]))
    s.append(("xyz", pts, [[r.uniform(-8, 8), r.uniform(-8, 8), r.uniform(4, 20)] for _ in pts]))
    return s, pts


def case_sum_order(v):
    """A float sum whose bits differ between key order and slot order: the first point sits at the
    origin, every other centre on the x axis (an x term of 1) and the rest just off the y axis (an
    x term near 2^-24), so the running x sum rounds a small term away, or not, by where it comes."""
    n = 5 + v
    s, pts = _world(2 * v, n, slots=2, octave=1)     # even variants: keys opposite to slots
    cs = []
    for i in range(n):
        if i % 2 == 0:
            cs.append([-1.0 - i, 0.0, 0.0])                    # x term 1
        else:
            # x term 2^-24 (1 + i + k), y term 1; k picked per size so that the two orders differ
            # after the mean as well (tests/test_refresh.py checks it)
            cs.append([-(2.0 ** -24) * (1 + i + (2, 2, 0, 0, 1)[v % 5]), -1.0, 0.0])
    s.append(("centers", [f"K{i}" for i in range(n)], cs))
    s.append(("xyz", pts, [[0.0, 0.0, 0.0], [0.5, 0.25, 0.125]]))
    s.append(("obsidx", [(p, f"K{i}", j) for i in range(n) for j, p in enumerate(pts)]))
    s.append(("refkf", pts, ["K1", f"K{n - 1}"]))
    s.append(("refresh", ND, pts))
    s.append(("refresh", ND | DESC, pts + [None, pts[0]]))
    return s


def case_median_tie(v):
    """Descriptors built so that two observers tie on the median; the keys run opposite to the
    slots, so the first in key order is the last in slot order."""
    n = 3 + v                                         # N = 3, 4, 5, ...: the median index at each
    s, pts = _world(2 * v, n, slots=3, octave=2)
    base = _desc_rows(77 + v, 1)[0]
    for i in range(n):
        d = np.tile(base, (3, 1))
        # slot 0: all equal; slot 1: one bit of its own per observer, so every pair is 2 apart
        # and every median ties while the descriptors differ; slot 2: random
        d[1, i % 32] ^= 1 << (i % 8)
        d[2] = _desc_rows(500 + 10 * v + i, 1)[0]
        s.append(("descs", f"K{i}", d))
    s.append(("obsidx", [(p, f"K{i}", j) for i in range(n) for j, p in enumerate(pts)]))
    s.append(("refkf", pts, ["K0", None, f"K{n - 1}"]))
    s.append(("refresh", DESC, pts))
    s.append(("kfbad", "K1", True))
    s.append(("refresh", ND | DESC, pts))
    return s


def case_refs(v):
    """The reference keyframe: NULL, bad, not an observer (index 0), without keypoints, at the top
    octave, beyond it (unsupported, in the middle of a list)."""
    n = 4
    s, pts = _world(2 * v + 1, n, slots=7, octave=None)
    s.append(("points", ["Q"]))
    s.append(("kf", "E", BASE + 0x77, []))            # no keypoints
    s.append(("kf", "T", BASE + 0x99 + v, [None, None]))
    s.append(("features", "T", [7, 8], None, None, 40.0))   # octave nlevels - 1, nlevels
    s.append(("descs", "T", _desc_rows(9 + v, 2)))
    s.append(("centers", ["E", "T"], [[1.0, 2.0, 3.0], [-2.0, 0.5, 1.0]]))
    s.append(("obsidx", [(p, f"K{i}", j) for i in range(n) for j, p in enumerate(pts) if (i + j) % 4 != 3]))
    s.append(("obsidx", [(pts[4], "T", 0), (pts[5], "T", 1)]))
    s.append(("kfbad", "K2", True))
    #          NULL  bad   absent  no keypoint  top   beyond  observer
    s.append(("refkf", pts, [None, "K2", "T", "E", "T", "T", "K0"]))
    s.append(("refresh", ND | DESC, pts))
    s.append(("refresh", ND, [pts[6], pts[5], pts[0], OOB]))
    s.append(("refresh", ND, [pts[6], pts[5], pts[4]]))
    s.append(("mpbad", [pts[1]], True))
    s.append(("refresh", ND | DESC, [pts[1], None, pts[2], pts[2]]))
    s.append(("refreshkf", "K0", ND | DESC))
    s.append(("refreshkf", "E", ND))
    s.append(("refresh", ND | DESC, ["Q"]))           # no observations
    return s


def case_bad_observers(v):
    """Bad keyframes: left out of the descriptor, counted for the normal; all bad: desc stays."""
    n = 4 + v
    s, pts = _world(2 * v, n, slots=4)
    s.append(("obsidx", [(p, f"K{i}", j) for i in range(n) for j, p in enumerate(pts)]))
    s.append(("refkf", pts, ["K0", "K1", "K2", "K3"]))
    s.append(("kfbad", "K0", True))
    s.append(("kfbad", f"K{n - 1}", True))
    s.append(("refresh", ND | DESC, pts))
    for i in range(n):
        s.append(("kfbad", f"K{i}", True))
    s.append(("refresh", ND | DESC, pts))
    return s


def case_erase_ref(v):
    """The three erase routes on the reference keyframe: the lowest key is not the lowest slot, the
    row runs empty, the point goes bad on that erase, a point held twice under SetBadFlag."""
    n = 5
    s, pts = _world(2 * v, n, slots=8, right_every=2 + v)
    # P0..P3 observed by all five; P4, P5 by K0, K1 only (they go bad when one leaves); P6 by K0 alone
    s.append(("obsidx", [(p, f"K{i}", j) for i in range(n) for j, p in enumerate(pts[:4])]))
    s.append(("obsidx", [(pts[4], "K0", 4), (pts[4], "K1", 4), (pts[5], "K0", 5), (pts[5], "K1", 5),
                         (pts[6], "K0", 6)]))
    s.append(("kfpoints", "K2", 7, [pts[0]]))         # K2 holds P0 twice: at 0 and at 7
    s.append(("obsidx", [(pts[7], "K3", 7)]))
    s.append(("refkf", pts, ["K0", "K1", "K2", "K0", "K0", "K1", "K0", "K3"]))
    s.append(("eraseobs", pts[0], "K0"))              # route 1: next is the lowest key
    s.append(("eraseobs", pts[4], "K0"))              # goes bad on that erase
    s.append(("eraseobs", pts[6], "K0"))              # the row runs empty
    s.append(("unobs", [(pts[1], "K1"), (pts[3], "K0"), (pts[3], "K4"), (pts[2], "K3"),
                        (pts[7], "K3")]))             # route 2; P7's row runs empty and it stays live
    s.append(("refresh", ND | DESC, pts))
    s.append(("kfbadflag", "K2"))                     # route 3: P0 held twice, P2's reference
    s.append(("refresh", ND | DESC, pts))
    s.append(("kfbadflag", "K1"))                     # P5 goes bad here, its reference is K1
    s.append(("refreshkf", "K3", ND | DESC))
    return s


def case_process(v):
    """ProcessNewKeyFrame: new, already observed, twice held, bad, NULL and stereo entries."""
    n = 4
    s, pts = _world(2 * v + 1, n, slots=6)
    s.append(("obsidx", [(p, f"K{i}", j) for i in range(n) for j, p in enumerate(pts)]))
    s.append(("refkf", pts, [f"K{j % n}" for j in range(len(pts))]))
    s.append(("points", ["S0", "S1"]))
    row = [pts[0], pts[1], None, pts[2], pts[1], "S0", pts[3], "S1", pts[0], pts[4]]
    s.append(("kf", "N", BASE + 0x33 + v, row))
    s.append(("features", "N", [j % 8 for j in range(len(row))],
              [1.0 if j % 2 == v % 2 else -1.0 for j in range(len(row))], None, 40.0))
    s.append(("descs", "N", _desc_rows(321 + v, len(row))))
    s.append(("centers", ["N"], [[0.25, -0.5, 0.75]]))
    s.append(("xyz", ["S0", "S1"], [[1.0, 1.0, 5.0], [-1.0, 2.0, 7.0]]))
    s.append(("obsidx", [("S0", "N", 5), ("S1", "N", 7)]))   # stereo points Tracking inserted
    s.append(("refkf", ["S0", "S1"], ["N", "N"]))
    s.append(("mpbad", [pts[3]], True))
    s.append(("process", "N", 2))                     # three recent: capacity, nothing changed
    s.append(("process", "N"))
    s.append(("process", "N"))                        # again: everything is observed by now
    return s


CASES = (case_sum_order, case_median_tie, case_refs, case_bad_observers, case_erase_ref, case_process)


def built_scripts():
    return [(f"{c.__name__[5:]}{v}", c(v)) for c in CASES for v in range(5)]


def script_observer_count(n, v=0, extra_slot=False):
    """One point observed by n keyframes of one slot each (keys ascending, descending or shuffled
    against the slots by v = 2, 0, 1), refreshed both ways; its reference is the middle one."""
    s = [("points", ["P", "Z"]), ("scale", SCALE8)]
    keys = sorted(keys_for(n, 0)) if v == 2 else keys_for(n, v)
    r = np.random.RandomState(n + 31 * v)
    base = r.randint(0, 256, 32).astype(np.uint8)
    cs = []
    for i in range(n):
        s.append(("kf", f"K{i}", keys[i], ["P"]))
        s.append(("features", f"K{i}", [i % 8], [-1.0], None, 40.0))
        d = base.copy()
        for b in r.randint(0, 256, 1 + i % 5):       # a few flipped bits: many equal medians
            d[b >> 3] ^= 1 << (b & 7)
        s.append(("descs", f"K{i}", d.reshape(1, 32)))
        cs.append([float(x) for x in r.uniform(-2, 2, 3)])
    if n:
        s.append(("centers", [f"K{i}" for i in range(n)], cs))
        s.append(("obsidx", [("P", f"K{i}", 0) for i in range(n)]))
        s.append(("refkf", ["P"], [f"K{n // 2}"]))
    s.append(("xyz", ["P"], [[0.5, -0.25, 9.0]]))
    s.append(("refresh", ND | DESC, ["P", "Z"]))
    return s


def script_list(n, v=0):
    """A list of n entries with -1, bad and repeated entries over a small map."""
    s, pts = _world(v, 4, slots=9)
    s.append(("obsidx", [(p, f"K{i}", j) for i in range(4) for j, p in enumerate(pts) if (i + j) % 5]))
    s.append(("refkf", pts, [f"K{j % 4}" for j in range(len(pts))]))
    s.append(("mpbad", [pts[2]], True))
    r = random.Random(n + v)
    s.append(("refresh", ND | DESC, [r.choice(pts + [None]) for _ in range(n)]))
    return s
