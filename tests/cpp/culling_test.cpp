// culling_test — the C++ adapter's culling (orbfe::LocalMap, include/orbfe_orbslam.hpp) against
// LocalMapping::MapPointCulling (LocalMapping.cc:170-205), LocalMapping::KeyFrameCulling (:632-698),
// MapPoint::AddObservation / EraseObservation / SetBadFlag (MapPoint.cc:339-409) and
// KeyFrame::SetBadFlag / SetErase (KeyFrame.cc:1158-1287) written out over heap-allocated stand-in
// structs with a real std::map<KF*, size_t>, std::set<KF*> and std::list<MP*>: the addresses are
// whatever the allocator gives, so "order_key = the pointer" is what is tested.
//
//   culling_test <seed>        a dense random map, its graph from UpdateConnections, then rounds of
//                              MapPointCulling, KeyFrameCulling over every keyframe's covisibility
//                              list, SetNotErase / SetErase and single erases; after every step the
//                              whole state of every keyframe and point is compared
//   culling_test --time [reps] times the literal loops alone at the bench shapes (30 listed
//                              keyframes x 1000 points, rows of about 8; 500 recent points); one
//                              thread, no device
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <list>
#include <map>
#include <random>
#include <set>
#include <vector>

#include "../../include/orbfe_orbslam.hpp"

namespace {

struct KF;
struct MP {
    uint64_t mnId = 0;
    bool mbBad = false;
    std::map<KF*, size_t> mObservations;
    int nObs = 0, mnFound = 1, mnVisible = 1;
    long mnFirstKFid = 0;
    bool isBad() const { return mbBad; }
    int Observations() const { return nObs; }
    float GetFoundRatio() const { return static_cast<float>(mnFound) / mnVisible; }
    void AddObservation(KF* pKF, size_t idx);
    void EraseObservation(KF* pKF);
    void SetBadFlag();
};

struct KF {
    uint64_t mnId = 0;
    std::vector<MP*> mvpMapPoints;
    std::vector<int> octave;  // mvKeysUn[i].octave
    std::vector<float> mvuRight, mvDepth;
    float mThDepth = 0;
    std::map<KF*, int> mConnectedKeyFrameWeights;
    std::vector<KF*> mvpOrderedConnectedKeyFrames;
    std::vector<int> mvOrderedWeights;
    bool mbFirstConnection = true, mbNotErase = false, mbToBeErased = false, mbBad = false;
    KF* mpParent = nullptr;
    std::set<KF*> mspChildrens;
    bool isBad() const { return mbBad; }

    void EraseMapPointMatch(size_t idx) { mvpMapPoints[idx] = nullptr; }
    void UpdateBestCovisibles() {
        std::vector<std::pair<int, KF*>> vPairs;
        for (auto& kv : mConnectedKeyFrameWeights) vPairs.push_back({kv.second, kv.first});
        std::sort(vPairs.begin(), vPairs.end());
        std::list<KF*> lKFs;
        std::list<int> lWs;
        for (auto& p : vPairs) {
            lKFs.push_front(p.second);
            lWs.push_front(p.first);
        }
        mvpOrderedConnectedKeyFrames.assign(lKFs.begin(), lKFs.end());
        mvOrderedWeights.assign(lWs.begin(), lWs.end());
    }
    void AddConnection(KF* pKF, int weight) {
        if (!mConnectedKeyFrameWeights.count(pKF)) mConnectedKeyFrameWeights[pKF] = weight;
        else if (mConnectedKeyFrameWeights[pKF] != weight) mConnectedKeyFrameWeights[pKF] = weight;
        else return;
        UpdateBestCovisibles();
    }
    void EraseConnection(KF* pKF) {
        bool bUpdate = false;
        if (mConnectedKeyFrameWeights.count(pKF)) {
            mConnectedKeyFrameWeights.erase(pKF);
            bUpdate = true;
        }
        if (bUpdate) UpdateBestCovisibles();
    }
    int GetWeight(KF* pKF) { return mConnectedKeyFrameWeights.count(pKF) ? mConnectedKeyFrameWeights[pKF] : 0; }
    void ChangeParent(KF* pKF) {
        mpParent = pKF;
        pKF->mspChildrens.insert(this);
    }
    void UpdateConnections() {
        std::map<KF*, int> KFcounter;
        for (MP* pMP : mvpMapPoints) {
            if (!pMP) continue;
            if (pMP->isBad()) continue;
            for (auto& ob : pMP->mObservations) {
                if (ob.first->mnId == mnId) continue;
                KFcounter[ob.first]++;
            }
        }
        if (KFcounter.empty()) return;
        int nmax = 0;
        KF* pKFmax = nullptr;
        std::vector<std::pair<int, KF*>> vPairs;
        for (auto& kv : KFcounter) {
            if (kv.second > nmax) {
                nmax = kv.second;
                pKFmax = kv.first;
            }
            if (kv.second >= 15) {
                vPairs.push_back({kv.second, kv.first});
                kv.first->AddConnection(this, kv.second);
            }
        }
        if (vPairs.empty()) {
            vPairs.push_back({nmax, pKFmax});
            pKFmax->AddConnection(this, nmax);
        }
        std::sort(vPairs.begin(), vPairs.end());
        std::list<KF*> lKFs;
        std::list<int> lWs;
        for (auto& p : vPairs) {
            lKFs.push_front(p.second);
            lWs.push_front(p.first);
        }
        mConnectedKeyFrameWeights = KFcounter;
        mvpOrderedConnectedKeyFrames.assign(lKFs.begin(), lKFs.end());
        mvOrderedWeights.assign(lWs.begin(), lWs.end());
        if (mbFirstConnection && mnId != 0) {
            mpParent = mvpOrderedConnectedKeyFrames.front();
            mpParent->mspChildrens.insert(this);
            mbFirstConnection = false;
        }
    }
    // KeyFrame.cc:1174-1287 without mTcp, Map::EraseKeyFrame and KeyFrameDatabase::erase
    void SetBadFlag(std::vector<MP*>* went_bad) {
        if (mnId == 0) return;
        else if (mbNotErase) {
            mbToBeErased = true;
            return;
        }
        for (auto& kv : mConnectedKeyFrameWeights) kv.first->EraseConnection(this);
        for (size_t i = 0; i < mvpMapPoints.size(); i++)
            if (mvpMapPoints[i]) {
                MP* p = mvpMapPoints[i];
                const bool was = p->mbBad || p->mObservations.count(this) == 0;
                p->EraseObservation(this);
                if (went_bad && !was && p->mbBad) went_bad->push_back(p);
            }
        mConnectedKeyFrameWeights.clear();
        mvpOrderedConnectedKeyFrames.clear();
        mvOrderedWeights.clear();  // not in the reference: nothing reads it past an empty list
        std::set<KF*> sParentCandidates;
        if (mpParent) sParentCandidates.insert(mpParent);
        while (!mspChildrens.empty()) {
            bool bContinue = false;
            int max = -1;
            KF* pC = nullptr;
            KF* pP = nullptr;
            for (KF* pKF : mspChildrens) {
                if (pKF->isBad()) continue;
                std::vector<KF*> vpConnected = pKF->mvpOrderedConnectedKeyFrames;
                for (size_t i = 0, iend = vpConnected.size(); i < iend; i++)
                    for (KF* cand : sParentCandidates)
                        if (vpConnected[i]->mnId == cand->mnId) {
                            int w = pKF->GetWeight(vpConnected[i]);
                            if (w > max) {
                                pC = pKF;
                                pP = vpConnected[i];
                                max = w;
                                bContinue = true;
                            }
                        }
            }
            if (bContinue) {
                pC->ChangeParent(pP);
                sParentCandidates.insert(pC);
                mspChildrens.erase(pC);
            } else
                break;
        }
        if (!mspChildrens.empty())
            for (KF* c : mspChildrens)
                if (mpParent) c->ChangeParent(mpParent);
        if (mpParent) mpParent->mspChildrens.erase(this);
        mbBad = true;
    }
    void SetErase(bool has_loop_edges, std::vector<MP*>* went_bad) {
        if (!has_loop_edges) mbNotErase = false;
        if (mbToBeErased) SetBadFlag(went_bad);
    }
};

void MP::AddObservation(KF* pKF, size_t idx) {
    if (mObservations.count(pKF)) return;
    mObservations[pKF] = idx;
    if (pKF->mvuRight[idx] >= 0) nObs += 2;
    else nObs++;
}
void MP::EraseObservation(KF* pKF) {
    bool bBad = false;
    if (mObservations.count(pKF)) {
        int idx = (int)mObservations[pKF];
        if (pKF->mvuRight[idx] >= 0) nObs -= 2;
        else nObs--;
        mObservations.erase(pKF);
        if (nObs <= 2) bBad = true;
    }
    if (bBad) SetBadFlag();
}
void MP::SetBadFlag() {
    std::map<KF*, size_t> obs;
    mbBad = true;
    obs = mObservations;
    mObservations.clear();
    for (auto& ob : obs) ob.first->EraseMapPointMatch(ob.second);
}

// LocalMapping.cc:170-205
void MapPointCulling(std::list<MP*>& mlpRecentAddedMapPoints, unsigned long nCurrentKFid, bool mbMonocular,
                     std::vector<MP*>* culled) {
    auto lit = mlpRecentAddedMapPoints.begin();
    const int cnThObs = mbMonocular ? 2 : 3;
    while (lit != mlpRecentAddedMapPoints.end()) {
        MP* pMP = *lit;
        if (pMP->isBad()) lit = mlpRecentAddedMapPoints.erase(lit);
        else if (pMP->GetFoundRatio() < 0.25f) {
            pMP->SetBadFlag();
            if (culled) culled->push_back(pMP);
            lit = mlpRecentAddedMapPoints.erase(lit);
        } else if (((int)nCurrentKFid - (int)pMP->mnFirstKFid) >= 2 && pMP->Observations() <= cnThObs) {
            pMP->SetBadFlag();
            if (culled) culled->push_back(pMP);
            lit = mlpRecentAddedMapPoints.erase(lit);
        } else if (((int)nCurrentKFid - (int)pMP->mnFirstKFid) >= 3) lit = mlpRecentAddedMapPoints.erase(lit);
        else lit++;
    }
}

// LocalMapping.cc:632-698
void KeyFrameCulling(KF* mpCurrentKeyFrame, bool mbMonocular, std::vector<KF*>* culled, std::vector<MP*>* went_bad) {
    std::vector<KF*> vpLocalKeyFrames = mpCurrentKeyFrame->mvpOrderedConnectedKeyFrames;
    for (KF* pKF : vpLocalKeyFrames) {
        if (pKF->mnId == 0) continue;
        const std::vector<MP*> vpMapPoints = pKF->mvpMapPoints;
        const int thObs = 3;
        int nRedundantObservations = 0, nMPs = 0;
        for (size_t i = 0, iend = vpMapPoints.size(); i < iend; i++) {
            MP* pMP = vpMapPoints[i];
            if (!pMP || pMP->isBad()) continue;
            if (!mbMonocular)
                if (pKF->mvDepth[i] > pKF->mThDepth || pKF->mvDepth[i] < 0) continue;
            nMPs++;
            if (pMP->Observations() > thObs) {
                const int scaleLevel = pKF->octave[i];
                const std::map<KF*, size_t> observations = pMP->mObservations;
                int nObs = 0;
                for (auto& ob : observations) {
                    KF* pKFi = ob.first;
                    if (pKFi == pKF) continue;
                    const int scaleLeveli = pKFi->octave[ob.second];
                    if (scaleLeveli <= scaleLevel + 1) {
                        nObs++;
                        if (nObs >= thObs) break;
                    }
                }
                if (nObs >= thObs) nRedundantObservations++;
            }
        }
        if (nRedundantObservations > 0.9 * nMPs) {
            const bool was = pKF->mbNotErase;
            pKF->SetBadFlag(went_bad);
            if (culled && !was) culled->push_back(pKF);
        }
    }
}

struct World {
    std::vector<KF*> kfs;
    std::vector<MP*> mps;
    ~World() {
        for (KF* k : kfs) delete k;
        for (MP* p : mps) delete p;
    }
};

// nkf keyframes of lo .. hi - 1 slots over npts shared points.  priv: the last `priv` slots of a
// keyframe hold points nobody else sees (none for keyframes full_a and full_b); flat: one octave,
// no right coordinates.
void build(World& w, std::mt19937& rng, int nkf, int npts, int lo, int hi, int priv = 0, int full_a = -1,
           int full_b = -1, bool flat = false) {
    auto rnd = [&](int n) { return (int)(rng() % (unsigned)n); };
    for (int i = 0; i < npts; ++i) {
        MP* p = new MP();
        p->mnId = 1000 + i;
        w.mps.push_back(p);
    }
    for (int i = 0; i < nkf; ++i) {
        KF* k = new KF();
        k->mnId = i;
        const int n = lo + rnd(hi - lo);
        for (int j = 0; j < n; ++j) {
            if (j >= n - priv && i != full_a && i != full_b) {
                MP* p = new MP();
                p->mnId = 1000 + w.mps.size();
                w.mps.push_back(p);
                k->mvpMapPoints.push_back(p);
            } else
                k->mvpMapPoints.push_back(rnd(20) ? w.mps[rnd(npts)] : nullptr);
            k->octave.push_back(flat || rnd(5) < 3 ? 0 : rnd(3));
            k->mvuRight.push_back(flat || rnd(2) ? -1.f : 3.5f);
            const float z[] = {0.5f, 1.f, 2.f, 3.f, 3.f, 2.5f, 3.5f, -1.f};
            k->mvDepth.push_back(z[rnd(8)]);
        }
        k->mThDepth = 3.f;
        w.kfs.push_back(k);
    }
    for (KF* k : w.kfs)
        for (size_t j = 0; j < k->mvpMapPoints.size(); ++j)
            if (k->mvpMapPoints[j] && rnd(30)) k->mvpMapPoints[j]->AddObservation(k, j);
    for (MP* p : w.mps) {
        p->mnFound = rnd(9);
        p->mnVisible = rnd(20);
        p->mnFirstKFid = rnd(nkf);
    }
}

int fails = 0;
#define EXPECT(c, ...)                                    \
    do {                                                  \
        if (!(c)) {                                       \
            if (fails++ < 10) std::printf(__VA_ARGS__);   \
        }                                                 \
    } while (0)

void compare(World& w, orbfe::LocalMap& lm, const char* step) {
    const uint64_t none = orbfe::LocalMap::kNone;
    for (KF* k : w.kfs) {
        const auto held = lm.GetMapPointMatches(k->mnId);
        bool same = held.size() == k->mvpMapPoints.size();
        for (size_t i = 0; same && i < held.size(); ++i)
            same = held[i] == (k->mvpMapPoints[i] ? k->mvpMapPoints[i]->mnId : none);
        EXPECT(same, "%s: mvpMapPoints of keyframe %d differ\n", step, (int)k->mnId);
        EXPECT(lm.KeyFrameIsBad(k->mnId) == k->mbBad, "%s: mbBad of keyframe %d\n", step, (int)k->mnId);
        EXPECT(lm.NotErase(k->mnId) == k->mbNotErase && lm.ToBeErased(k->mnId) == k->mbToBeErased,
               "%s: erase flags of keyframe %d\n", step, (int)k->mnId);
        EXPECT(lm.GetParent(k->mnId) == (k->mpParent ? k->mpParent->mnId : none), "%s: parent of keyframe %d\n", step,
               (int)k->mnId);
        std::vector<uint64_t> ch, conn, ord;
        for (KF* c : k->mspChildrens) ch.push_back(c->mnId);
        for (auto& kv : k->mConnectedKeyFrameWeights) conn.push_back(kv.first->mnId);
        for (KF* c : k->mvpOrderedConnectedKeyFrames) ord.push_back(c->mnId);
        EXPECT(lm.GetChilds(k->mnId) == ch, "%s: children of keyframe %d\n", step, (int)k->mnId);
        EXPECT(lm.GetConnectedKeyFrames(k->mnId) == conn, "%s: weight map of keyframe %d\n", step, (int)k->mnId);
        EXPECT(lm.GetVectorCovisibleKeyFrames(k->mnId) == ord, "%s: ordered list of keyframe %d\n", step, (int)k->mnId);
        EXPECT(lm.GetOrderedWeights(k->mnId) == k->mvOrderedWeights, "%s: ordered weights of keyframe %d\n", step,
               (int)k->mnId);
    }
    for (MP* p : w.mps) {
        EXPECT(lm.MapPointIsBad(p->mnId) == p->mbBad, "%s: mbBad of point %d\n", step, (int)p->mnId);
        EXPECT(lm.Observations(p->mnId) == p->nObs, "%s: nObs of point %d: %d, reference %d\n", step, (int)p->mnId,
               lm.Observations(p->mnId), p->nObs);
        std::map<uint64_t, int64_t> a, b;
        for (auto& ob : lm.GetObservations(p->mnId)) a[ob.first] = ob.second;
        for (auto& ob : p->mObservations) b[ob.first->mnId] = (int64_t)ob.second;
        EXPECT(a == b, "%s: observations of point %d\n", step, (int)p->mnId);
    }
}

std::vector<uint64_t> ids(const std::vector<MP*>& v) {
    std::vector<uint64_t> o;
    for (MP* p : v) o.push_back(p->mnId);
    return o;
}

int run(unsigned seed) {
    std::mt19937 rng(seed);
    auto rnd = [&](int n) { return (int)(rng() % (unsigned)n); };
    World w;
    build(w, rng, 10, 48, 30, 42, 0, -1, -1, seed % 2 == 0);  // even seeds: one octave, dense culls
    orbfe::LocalMap lm(0);
    for (MP* p : w.mps) lm.NewMapPoint(p->mnId);
    for (KF* k : w.kfs) {
        std::vector<uint64_t> held;
        for (MP* p : k->mvpMapPoints) held.push_back(p ? p->mnId : orbfe::LocalMap::kNone);
        lm.NewKeyFrame(k->mnId, (uint64_t)(uintptr_t)k, held);
        lm.SetKeyFrameFeatures(k->mnId, std::vector<int32_t>(k->octave.begin(), k->octave.end()), k->mvuRight,
                               k->mvDepth, k->mThDepth);
    }
    for (MP* p : w.mps) {
        for (auto& ob : p->mObservations) lm.AddObservation(p->mnId, ob.first->mnId, ob.second);
        lm.IncreaseFound(p->mnId, p->mnFound - 1);
        lm.IncreaseVisible(p->mnId, p->mnVisible - 1);
        lm.SetFirstKFid(p->mnId, p->mnFirstKFid);
    }
    std::vector<uint64_t> all;
    for (KF* k : w.kfs) {
        k->UpdateConnections();
        all.push_back(k->mnId);
    }
    lm.UpdateConnections(all);
    compare(w, lm, "built");
    int multi = 0;
    for (int step = 0; step < 8 && !fails; ++step) {
        char name[64];
        const int what = step == 0 ? 0 : rnd(6);
        KF* k = w.kfs[(size_t)rnd((int)w.kfs.size())];
        if (what == 0) {  // MapPointCulling over a recent list with repeats
            std::list<MP*> recent;
            std::list<uint64_t> recent_ids;
            for (int i = 0; i < 30; ++i) {
                recent.push_back(w.mps[(size_t)rnd((int)w.mps.size())]);
                recent_ids.push_back(recent.back()->mnId);
            }
            std::vector<MP*> culled;
            const int cur = rnd(9);
            const bool mono = rnd(2);
            MapPointCulling(recent, (unsigned long)cur, mono, &culled);
            const auto got = lm.MapPointCulling(recent_ids, (uint64_t)cur, mono);
            std::list<uint64_t> want;
            for (MP* p : recent) want.push_back(p->mnId);
            EXPECT(recent_ids == want, "step %d: the recent list differs\n", step);
            EXPECT(got == ids(culled), "step %d: the culled points differ\n", step);
            std::snprintf(name, sizeof name, "step %d MapPointCulling", step);
        } else if (what <= 3) {
            std::vector<KF*> culled;
            std::vector<MP*> went_bad;
            const bool mono = rnd(2);
            KeyFrameCulling(k, mono, &culled, &went_bad);
            const auto r = lm.KeyFrameCulling(k->mnId, mono);
            std::vector<uint64_t> c;
            for (KF* x : culled) c.push_back(x->mnId);
            EXPECT(r.culled == c, "step %d: the culled keyframes differ (%zu, reference %zu)\n", step, r.culled.size(),
                   c.size());
            EXPECT(r.bad_points == ids(went_bad), "step %d: the points that went bad differ\n", step);
            multi += c.size() >= 2;
            std::snprintf(name, sizeof name, "step %d KeyFrameCulling", step);
        } else if (what == 4) {
            if (rnd(2)) {
                k->mbNotErase = true;
                lm.SetNotErase(k->mnId);
            } else {
                std::vector<MP*> went_bad;
                const bool loop = rnd(3) == 0;
                k->SetErase(loop, &went_bad);
                const auto r = lm.SetErase(k->mnId, loop, k->mnId == 0);
                EXPECT(r.bad_points == ids(went_bad), "step %d: SetErase's bad points differ\n", step);
            }
            std::snprintf(name, sizeof name, "step %d SetNotErase / SetErase", step);
        } else {
            MP* p = w.mps[(size_t)rnd((int)w.mps.size())];
            p->EraseObservation(k);
            bool bad = false;
            lm.EraseObservation(p->mnId, k->mnId, &bad);
            EXPECT(!bad || p->mbBad, "step %d: EraseObservation's went_bad\n", step);
            std::snprintf(name, sizeof name, "step %d EraseObservation", step);
        }
        compare(w, lm, name);
    }
    std::printf("culling_test seed %u: %s (%d calls culled two or more keyframes)\n", seed, fails ? "FAIL" : "ok", multi);
    return fails ? 1 : 0;
}

int time_loops(int reps) {
    using clk = std::chrono::steady_clock;
    double best_kf[2] = {1e30, 1e30}, best_mp = 1e30;
    for (int variant = 0; variant < 2; ++variant)
        for (int r = 0; r < reps; ++r) {
            std::mt19937 rng(7);
            World w;
            // 850 shared slots over 3,300 points (rows of about 8) and 150 private ones: 85 % redundant
            // at most, kept; variant 1: keyframes 10 and 20 have no private points and go
            build(w, rng, 31, 3300, 1000, 1001, 150, variant ? 10 : -1, variant ? 20 : -1, true);
            for (KF* k : w.kfs) k->UpdateConnections();
            KF* cur = w.kfs.back();
            cur->mvpOrderedConnectedKeyFrames.assign(w.kfs.begin() + 1, w.kfs.end() - 1);
            cur->mvpOrderedConnectedKeyFrames.push_back(w.kfs[0]);
            std::vector<KF*> culled;
            const auto t0 = clk::now();
            KeyFrameCulling(cur, true, &culled, nullptr);
            const double us = std::chrono::duration<double, std::micro>(clk::now() - t0).count();
            best_kf[variant] = std::min(best_kf[variant], us);
            if (r == 0) std::printf("KeyFrameCulling variant %d: %zu culled\n", variant, culled.size());
            if (variant == 0) {
                std::list<MP*> recent(w.mps.begin(), w.mps.begin() + 500);
                const auto t1 = clk::now();
                MapPointCulling(recent, 4, false, nullptr);
                best_mp = std::min(best_mp, std::chrono::duration<double, std::micro>(clk::now() - t1).count());
            }
        }
    std::printf("literal KeyFrameCulling, 30 x 1000, none culled: %.1f us; two culled: %.1f us\n", best_kf[0], best_kf[1]);
    std::printf("literal MapPointCulling, 500 points: %.1f us\n", best_mp);
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc >= 2 && std::string(argv[1]) == "--time") return time_loops(argc >= 3 ? std::atoi(argv[2]) : 5);
    const unsigned seed = argc >= 2 ? (unsigned)std::strtoul(argv[1], nullptr, 10) : 1;
    try {
        return run(seed);
    } catch (const std::exception& e) {
        std::printf("culling_test: %s\n", e.what());
        return 2;
    }
}
