// localmap_test — the C++ adapter's LocalMap (include/orbfe_orbslam.hpp) against
// Tracking::UpdateLocalKeyFrames / UpdateLocalPoints (Tracking.cc:1465-1599) written out over
// heap-allocated stand-in KeyFrame / MapPoint structs with a real std::map<KF*, int> and
// std::set<KF*>: the addresses are whatever the allocator gives, so "order_key = the pointer" is
// what is tested.
//
//   localmap_test <seed> [updates]           a seeded map and a walk of mutations and updates; after
//                                            every update the keyframe list, the reference
//                                            keyframe, the point list, the frame's points and
//                                            every stamp are compared
//   localmap_test --time [reps]              times the std::map loop alone at the config-5 shape
//                                            (1000 frame points, ~60 local keyframes of 2000
//                                            slots, ~50k distinct points); one thread, no device
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>
#include <set>
#include <vector>

#include "../../include/orbfe_orbslam.hpp"

namespace {

struct KF;
struct MP {
    uint64_t mnId;
    bool bad = false;
    unsigned long mnTrackReferenceForFrame = 0;
    std::map<KF*, size_t> mObservations;
    bool isBad() const { return bad; }
};
struct KF {
    uint64_t mnId;
    bool bad = false;
    unsigned long mnTrackReferenceForFrame = 0;
    std::vector<MP*> mvpMapPoints;
    std::vector<KF*> mvpOrderedConnectedKeyFrames;
    std::set<KF*> mspChildrens;
    KF* mpParent = nullptr;
    bool isBad() const { return bad; }
    std::vector<KF*> GetBestCovisibilityKeyFrames(int N) const {
        if ((int)mvpOrderedConnectedKeyFrames.size() < N) return mvpOrderedConnectedKeyFrames;
        return std::vector<KF*>(mvpOrderedConnectedKeyFrames.begin(), mvpOrderedConnectedKeyFrames.begin() + N);
    }
};

struct Tracker {
    std::vector<KF*> mvpLocalKeyFrames;
    std::vector<MP*> mvpLocalMapPoints;
    KF* mpReferenceKF = nullptr;

    void UpdateLocalPoints(unsigned long frameId) {
        mvpLocalMapPoints.clear();
        for (KF* pKF : mvpLocalKeyFrames) {
            for (MP* pMP : pKF->mvpMapPoints) {
                if (!pMP) continue;
                if (pMP->mnTrackReferenceForFrame == frameId) continue;
                if (!pMP->isBad()) {
                    mvpLocalMapPoints.push_back(pMP);
                    pMP->mnTrackReferenceForFrame = frameId;
                }
            }
        }
    }

    void UpdateLocalKeyFrames(unsigned long frameId, std::vector<MP*>& frame) {
        std::map<KF*, int> keyframeCounter;
        for (size_t i = 0; i < frame.size(); i++) {
            if (frame[i]) {
                MP* pMP = frame[i];
                if (!pMP->isBad()) {
                    for (const auto& ob : pMP->mObservations) keyframeCounter[ob.first]++;
                } else {
                    frame[i] = nullptr;
                }
            }
        }
        if (keyframeCounter.empty()) return;
        int max = 0;
        KF* pKFmax = nullptr;
        mvpLocalKeyFrames.clear();
        mvpLocalKeyFrames.reserve(3 * keyframeCounter.size());
        for (const auto& it : keyframeCounter) {
            KF* pKF = it.first;
            if (pKF->isBad()) continue;
            if (it.second > max) {
                max = it.second;
                pKFmax = pKF;
            }
            mvpLocalKeyFrames.push_back(pKF);
            pKF->mnTrackReferenceForFrame = frameId;
        }
        // the end iterator is taken before any push (the reserve keeps it valid): by index here
        const size_t end = mvpLocalKeyFrames.size();
        for (size_t k = 0; k < end; k++) {
            if (mvpLocalKeyFrames.size() > 80) break;
            KF* pKF = mvpLocalKeyFrames[k];
            for (KF* pNeighKF : pKF->GetBestCovisibilityKeyFrames(10)) {
                if (!pNeighKF->isBad()) {
                    if (pNeighKF->mnTrackReferenceForFrame != frameId) {
                        mvpLocalKeyFrames.push_back(pNeighKF);
                        pNeighKF->mnTrackReferenceForFrame = frameId;
                        break;
                    }
                }
            }
            for (KF* pChildKF : pKF->mspChildrens) {
                if (!pChildKF->isBad()) {
                    if (pChildKF->mnTrackReferenceForFrame != frameId) {
                        mvpLocalKeyFrames.push_back(pChildKF);
                        pChildKF->mnTrackReferenceForFrame = frameId;
                        break;
                    }
                }
            }
            KF* pParent = pKF->mpParent;
            if (pParent) {
                if (pParent->mnTrackReferenceForFrame != frameId) {
                    mvpLocalKeyFrames.push_back(pParent);
                    pParent->mnTrackReferenceForFrame = frameId;
                    break;
                }
            }
        }
        if (pKFmax) mpReferenceKF = pKFmax;
    }

    void UpdateLocalMap(unsigned long frameId, std::vector<MP*>& frame) {
        UpdateLocalKeyFrames(frameId, frame);
        UpdateLocalPoints(frameId);
    }
};

struct World {
    std::vector<KF*> kfs;
    std::vector<MP*> mps;
    ~World() {
        for (KF* k : kfs) delete k;
        for (MP* p : mps) delete p;
    }
};

// keyframes allocated in an order unrelated to their ids, with allocations of other sizes in
// between, so that address order and id (slot) order disagree
void build(World& w, std::mt19937& rng, int nkf, int npts, int slots, int nobs_extra) {
    for (int i = 0; i < npts; ++i) {
        w.mps.push_back(new MP());
        w.mps.back()->mnId = 1000 + i;
    }
    std::vector<KF*> alloc;
    std::vector<void*> junk;
    for (int i = 0; i < nkf; ++i) {
        alloc.push_back(new KF());
        if (rng() % 3 == 0) junk.push_back(std::malloc(16 + rng() % 200));
    }
    std::shuffle(alloc.begin(), alloc.end(), rng);
    for (void* j : junk) std::free(j);
    for (int i = 0; i < nkf; ++i) {
        KF* k = alloc[i];
        k->mnId = 7 + 3 * i;
        w.kfs.push_back(k);
        const int n = slots ? (int)(rng() % (unsigned)slots) : 0;
        for (int s = 0; s < n; ++s) {
            MP* p = rng() % 5 ? w.mps[rng() % w.mps.size()] : nullptr;
            k->mvpMapPoints.push_back(p);
            if (p) p->mObservations.emplace(k, (size_t)s);
        }
    }
    for (int i = 0; i < nobs_extra; ++i)
        w.mps[rng() % w.mps.size()]->mObservations.emplace(w.kfs[rng() % w.kfs.size()], 0);
    for (KF* k : w.kfs) {
        const int nc = (int)(rng() % 13);
        for (int j = 0; j < nc; ++j) k->mvpOrderedConnectedKeyFrames.push_back(w.kfs[rng() % w.kfs.size()]);
        const int nch = (int)(rng() % 4);
        for (int j = 0; j < nch; ++j) k->mspChildrens.insert(w.kfs[rng() % w.kfs.size()]);
        if (rng() % 3) k->mpParent = w.kfs[rng() % w.kfs.size()];
    }
}

int time_mode(int reps) {
    std::mt19937 rng(5);
    World w;
    const int nkf = 60, per = 2000, npts = 50000;
    for (int i = 0; i < npts; ++i) w.mps.push_back(new MP());
    for (int i = 0; i < nkf; ++i) w.kfs.push_back(new KF());
    for (int i = 0; i < nkf; ++i) {
        KF* k = w.kfs[i];
        for (int s = 0; s < per; ++s) {
            // a sliding window over the points: neighbours share, ~50k distinct in all
            MP* p = w.mps[(size_t)((long long)i * (npts - per) / (nkf - 1) + (rng() % per)) % npts];
            k->mvpMapPoints.push_back(p);
            p->mObservations.emplace(k, (size_t)s);
        }
        for (int j = 1; j <= 10; ++j) k->mvpOrderedConnectedKeyFrames.push_back(w.kfs[(i + j) % nkf]);
        if (i) k->mpParent = w.kfs[i - 1];
    }
    std::vector<MP*> frame0(1000);
    for (auto& p : frame0) p = rng() % 4 ? w.mps[rng() % npts] : nullptr;
    Tracker t;
    size_t nk = 0, np = 0;
    const auto t0 = std::chrono::steady_clock::now();
    for (int r = 0; r < reps; ++r) {
        std::vector<MP*> frame = frame0;
        t.UpdateLocalMap(100 + r, frame);
        nk = t.mvpLocalKeyFrames.size();
        np = t.mvpLocalMapPoints.size();
    }
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    std::printf("TIME keyframes=%zu points=%zu ms_per_call=%.6f\n", nk, np, ms / reps);
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc >= 2 && std::strcmp(argv[1], "--time") == 0)
        return time_mode(argc >= 3 ? std::atoi(argv[2]) : 20);
    const unsigned seed = argc >= 2 ? (unsigned)std::atoi(argv[1]) : 1;
    const int updates = argc >= 3 ? std::atoi(argv[2]) : 40;
    try {
        std::mt19937 rng(seed);
        World w;
        build(w, rng, 90 + seed % 7, 1500, 48, 300);
        int inversions = 0;  // address order against id order
        for (size_t i = 1; i < w.kfs.size(); ++i) inversions += w.kfs[i] < w.kfs[i - 1];
        orbfe::LocalMap lm(0);
        const uint64_t none = orbfe::LocalMap::kNone;
        std::map<uint64_t, KF*> kf_of;
        std::map<uint64_t, MP*> mp_of;
        for (MP* p : w.mps) {
            lm.NewMapPoint(p->mnId);
            mp_of[p->mnId] = p;
        }
        for (KF* k : w.kfs) {
            std::vector<uint64_t> mps;
            for (MP* p : k->mvpMapPoints) mps.push_back(p ? p->mnId : none);
            lm.NewKeyFrame(k->mnId, (uint64_t)(uintptr_t)k, mps);
            kf_of[k->mnId] = k;
        }
        for (MP* p : w.mps)
            for (const auto& ob : p->mObservations) lm.AddObservation(p->mnId, ob.first->mnId);
        for (KF* k : w.kfs) {
            std::vector<uint64_t> ord;
            for (KF* n : k->mvpOrderedConnectedKeyFrames) ord.push_back(n->mnId);
            lm.UpdateBestCovisibles(k->mnId, ord);
            for (KF* c : k->mspChildrens) lm.AddChild(k->mnId, c->mnId);
            if (k->mpParent) lm.SetParent(k->mnId, k->mpParent->mnId);
        }
        Tracker t;
        int bad = 0, nonempty = 0;
        unsigned long frameId = 1;
        for (int u = 0; u < updates; ++u) {
            // mutations through the adapter's hooks
            for (int j = 0; j < 6; ++j) {
                KF* k = w.kfs[rng() % w.kfs.size()];
                MP* p = w.mps[rng() % w.mps.size()];
                switch (rng() % 6) {
                    case 0: k->bad = true; lm.SetKeyFrameBadFlag(k->mnId); break;
                    case 1: p->bad = true; lm.SetBadFlag(p->mnId); break;
                    case 2: if (!p->mObservations.count(k)) p->mObservations[k] = 0;
                            lm.AddObservation(p->mnId, k->mnId); break;
                    case 3: p->mObservations.erase(k); lm.EraseObservation(p->mnId, k->mnId); break;
                    case 4: if (!k->mvpMapPoints.empty()) {
                                const size_t idx = rng() % k->mvpMapPoints.size();
                                k->mvpMapPoints[idx] = p;
                                lm.AddMapPoint(k->mnId, idx, p->mnId);
                            } break;
                    default: {
                        KF* par = w.kfs[rng() % w.kfs.size()];
                        k->mpParent = par;           // KeyFrame::ChangeParent
                        par->mspChildrens.insert(k);
                        lm.ChangeParent(k->mnId, par->mnId);
                    }
                }
            }
            frameId += rng() % 2;  // sometimes the same frame id again
            const int n = (int)(rng() % 4 ? rng() % 130 : 0);
            std::vector<MP*> frame(n);
            std::vector<uint64_t> ids(n);
            for (int i = 0; i < n; ++i) {
                frame[i] = rng() % 4 ? w.mps[rng() % w.mps.size()] : nullptr;
                ids[i] = frame[i] ? frame[i]->mnId : none;
            }
            t.UpdateLocalMap(frameId, frame);
            const orbfe::LocalMap::Result r = lm.UpdateLocalMap(frameId, ids);
            bool ok = r.mvpLocalKeyFrames.size() == t.mvpLocalKeyFrames.size() &&
                      r.mvpLocalMapPoints.size() == t.mvpLocalMapPoints.size() &&
                      r.mpReferenceKF == (t.mpReferenceKF ? t.mpReferenceKF->mnId : none);
            for (size_t i = 0; ok && i < r.mvpLocalKeyFrames.size(); ++i)
                ok = r.mvpLocalKeyFrames[i] == t.mvpLocalKeyFrames[i]->mnId;
            for (size_t i = 0; ok && i < r.mvpLocalMapPoints.size(); ++i)
                ok = r.mvpLocalMapPoints[i] == t.mvpLocalMapPoints[i]->mnId;
            for (int i = 0; ok && i < n; ++i) ok = ids[i] == (frame[i] ? frame[i]->mnId : none);
            for (size_t i = 0; ok && i < w.kfs.size(); ++i)
                ok = lm.KeyFrameStamp(w.kfs[i]->mnId) == w.kfs[i]->mnTrackReferenceForFrame;
            for (size_t i = 0; ok && i < w.mps.size(); i += 7)
                ok = lm.MapPointStamp(w.mps[i]->mnId) == w.mps[i]->mnTrackReferenceForFrame;
            if (!ok) ++bad;
            nonempty += !t.mvpLocalMapPoints.empty();
            std::printf("U %d frame=%lu n=%d kfs=%zu pts=%zu %s\n", u, frameId, n,
                        t.mvpLocalKeyFrames.size(), t.mvpLocalMapPoints.size(), ok ? "ok" : "MISMATCH");
        }
        std::printf("LOCALMAP DONE updates=%d nonempty=%d inversions=%d bad=%d\n", updates, nonempty,
                    inversions, bad);
        return bad ? 1 : 0;
    } catch (const std::exception& e) {
        std::printf("ERROR %s\n", e.what());
        return 2;
    }
}
