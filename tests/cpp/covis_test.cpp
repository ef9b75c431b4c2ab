// covis_test — the C++ adapter's covisibility graph (orbfe::LocalMap, include/orbfe_orbslam.hpp)
// against KeyFrame::UpdateConnections / AddConnection / UpdateBestCovisibles / EraseConnection /
// GetCovisiblesByWeight (KeyFrame.cc:844-929, 1010-1100, 1295-1309) written out over heap-allocated
// stand-in structs with a real std::map<KF*, int>, std::vector and std::list: the addresses are
// whatever the allocator gives, so "order_key = the pointer" is what is tested.
//
//   covis_test <seed>        the online sequence (a new keyframe, UpdateConnections, fuse-like
//                            edits, UpdateConnections again), the load-map loop (UpdateConnections
//                            on every keyframe in turn, System.cc:188-191) and
//                            GetCovisiblesByWeight at its quirk; after every step the whole graph
//                            of every keyframe is compared
//   covis_test --time [reps] times the literal loop alone at the two bench shapes: the online call
//                            on 60 keyframes x 2000 slots over 50,000 points, and the load-map
//                            loop over 1000 keyframes x 1000 slots; one thread, no device
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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
    bool bad = false;
    std::map<KF*, size_t> mObservations;
    bool isBad() const { return bad; }
};

struct KF {
    uint64_t mnId = 0;
    std::vector<MP*> mvpMapPoints;
    std::map<KF*, int> mConnectedKeyFrameWeights;
    std::vector<KF*> mvpOrderedConnectedKeyFrames;
    std::vector<int> mvOrderedWeights;
    bool mbFirstConnection = true;
    KF* mpParent = nullptr;
    std::set<KF*> mspChildrens;

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
        const int th = 15;
        std::vector<std::pair<int, KF*>> vPairs;
        for (auto& kv : KFcounter) {
            if (kv.second > nmax) {
                nmax = kv.second;
                pKFmax = kv.first;
            }
            if (kv.second >= th) {
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
    static bool weightComp(int a, int b) { return a > b; }
    std::vector<KF*> GetCovisiblesByWeight(int w) {
        if (mvpOrderedConnectedKeyFrames.empty()) return {};
        auto it = std::upper_bound(mvOrderedWeights.begin(), mvOrderedWeights.end(), w, weightComp);
        if (it == mvOrderedWeights.end()) return {};
        const int n = (int)(it - mvOrderedWeights.begin());
        return std::vector<KF*>(mvpOrderedConnectedKeyFrames.begin(), mvpOrderedConnectedKeyFrames.begin() + n);
    }
};

struct World {
    std::vector<KF*> kfs;
    std::vector<MP*> mps;
};

// nkf keyframes of `per` slots in a sliding window over npts points; addresses shuffled against ids
void build(World& w, std::mt19937& rng, int nkf, int per, int npts, int span, bool shuffle, bool nulls = true) {
    for (int i = 0; i < npts; ++i) {
        w.mps.push_back(new MP());
        w.mps.back()->mnId = 100 + i;
    }
    std::vector<KF*> alloc;
    for (int i = 0; i < nkf; ++i) alloc.push_back(new KF());
    if (shuffle) std::shuffle(alloc.begin(), alloc.end(), rng);
    for (int i = 0; i < nkf; ++i) {
        KF* k = alloc[i];
        k->mnId = (uint64_t)i;
        w.kfs.push_back(k);
        const long long lo = nkf > 1 ? (long long)i * (npts - span) / (nkf - 1) : 0;
        for (int s = 0; s < per; ++s) {
            MP* p = !nulls || rng() % 16 ? w.mps[(size_t)(lo + rng() % span)] : nullptr;
            k->mvpMapPoints.push_back(p);
            if (p) p->mObservations.emplace(k, (size_t)s);
        }
    }
}

int time_mode(int reps) {
    {
        std::mt19937 rng(5);
        World w;
        build(w, rng, 60, 2000, 50000, 2000, false, false);  // the config-5 map of tools/bench_rows.py
        for (KF* k : w.kfs) k->UpdateConnections();
        size_t n = 0;
        const auto t0 = std::chrono::steady_clock::now();
        for (int r = 0; r < reps; ++r)
            for (KF* k : w.kfs) {
                k->UpdateConnections();
                n += k->mConnectedKeyFrameWeights.size();
            }
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        std::printf("TIME online keyframes=60 slots=2000 neighbours=%.1f ms_per_call=%.6f\n",
                    (double)n / (60.0 * reps), ms / (60.0 * reps));
    }
    {
        std::mt19937 rng(6);
        World w;
        build(w, rng, 1000, 1000, 100000, 1000, false, false);
        size_t n = 0;
        double best = 1e30;
        for (int r = 0; r < std::max(reps / 4, 2); ++r) {
            const auto t0 = std::chrono::steady_clock::now();
            for (KF* k : w.kfs) k->UpdateConnections();  // System.cc:188-191
            best = std::min(best, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
        }
        for (KF* k : w.kfs) n += k->mConnectedKeyFrameWeights.size();
        std::printf("TIME loadmap keyframes=1000 slots=1000 neighbours=%.1f ms_per_call=%.6f\n", (double)n / 1000.0, best);
    }
    return 0;
}

// the whole graph of every keyframe, adapter against the structs
int compare(orbfe::LocalMap& lm, const World& w, const char* what) {
    int bad = 0;
    const uint64_t none = orbfe::LocalMap::kNone;
    for (KF* k : w.kfs) {
        bool ok = true;
        std::vector<uint64_t> keys;
        for (auto& kv : k->mConnectedKeyFrameWeights) keys.push_back(kv.first->mnId);
        ok = ok && lm.GetConnectedKeyFrames(k->mnId) == keys;
        for (auto& kv : k->mConnectedKeyFrameWeights) ok = ok && lm.GetWeight(k->mnId, kv.first->mnId) == kv.second;
        std::vector<uint64_t> ord;
        for (KF* o : k->mvpOrderedConnectedKeyFrames) ord.push_back(o->mnId);
        ok = ok && lm.GetVectorCovisibleKeyFrames(k->mnId) == ord;
        ok = ok && lm.GetOrderedWeights(k->mnId) == k->mvOrderedWeights;
        ok = ok && lm.GetParent(k->mnId) == (k->mpParent ? k->mpParent->mnId : none);
        std::vector<uint64_t> ch;
        for (KF* c : k->mspChildrens) ch.push_back(c->mnId);
        ok = ok && lm.GetChilds(k->mnId) == ch;
        ok = ok && lm.FirstConnection(k->mnId) == k->mbFirstConnection;
        for (int wt : {1, 15, 16, 40}) {
            std::vector<uint64_t> by;
            for (KF* o : k->GetCovisiblesByWeight(wt)) by.push_back(o->mnId);
            ok = ok && lm.GetCovisiblesByWeight(k->mnId, wt) == by;
        }
        std::vector<uint64_t> best(ord.begin(), ord.begin() + std::min<size_t>(ord.size(), 10));
        ok = ok && lm.GetBestCovisibilityKeyFrames(k->mnId, 10) == best;
        if (!ok) {
            ++bad;
            std::printf("MISMATCH %s keyframe %llu\n", what, (unsigned long long)k->mnId);
        }
    }
    return bad;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc >= 2 && std::strcmp(argv[1], "--time") == 0)
        return time_mode(argc >= 3 ? std::atoi(argv[2]) : 8);
    const unsigned seed = argc >= 2 ? (unsigned)std::atoi(argv[1]) : 1;
    try {
        std::mt19937 rng(seed);
        World w;
        const int nkf = 24 + (int)(seed % 5);
        build(w, rng, nkf, 120, 900, 220, true);
        int inversions = 0;
        for (size_t i = 1; i < w.kfs.size(); ++i) inversions += w.kfs[i] < w.kfs[i - 1];
        const uint64_t none = orbfe::LocalMap::kNone;
        orbfe::LocalMap lm(0);
        for (MP* p : w.mps) lm.NewMapPoint(p->mnId);
        // asymmetries: held without being observed, observed without being held, a bad point
        for (int j = 0; j < 40; ++j) {
            KF* k = w.kfs[rng() % w.kfs.size()];
            MP* p = w.mps[rng() % w.mps.size()];
            if (j % 2) p->mObservations.erase(k);
            else p->mObservations.emplace(k, 0);
        }
        for (int j = 0; j < 10; ++j) w.mps[rng() % w.mps.size()]->bad = true;
        int bad = 0, steps = 0, quirk = 0, resorted = 0;
        // ---- the online sequence
        World seen;
        seen.mps = w.mps;
        for (KF* k : w.kfs) {
            std::vector<uint64_t> mps;
            for (MP* p : k->mvpMapPoints) mps.push_back(p ? p->mnId : none);
            lm.NewKeyFrame(k->mnId, (uint64_t)(uintptr_t)k, mps);
            seen.kfs.push_back(k);
        }
        for (MP* p : w.mps) {
            if (p->bad) lm.SetBadFlag(p->mnId);
            for (auto& ob : p->mObservations) lm.AddObservation(p->mnId, ob.first->mnId);
        }
        for (KF* k : w.kfs) {
            k->UpdateConnections();
            lm.UpdateConnections(k->mnId);
            bad += compare(lm, w, "online");
            ++steps;
            // fuse-like edits: points replaced in the keyframe, observations moved
            for (int j = 0; j < 12; ++j) {
                const size_t idx = rng() % k->mvpMapPoints.size();
                MP* p = w.mps[rng() % w.mps.size()];
                k->mvpMapPoints[idx] = p;
                lm.AddMapPoint(k->mnId, idx, p->mnId);
                if (rng() % 2) {
                    p->mObservations.emplace(k, idx);
                    lm.AddObservation(p->mnId, k->mnId);
                }
            }
            k->UpdateConnections();
            lm.UpdateConnections(k->mnId);
            bad += compare(lm, w, "online, after edits");
            ++steps;
        }
        for (KF* k : w.kfs) {
            resorted += k->mvpOrderedConnectedKeyFrames.size() == k->mConnectedKeyFrameWeights.size() &&
                        !k->mvOrderedWeights.empty() && k->mvOrderedWeights.back() < 15 &&
                        k->mvOrderedWeights.size() > 1;
            for (int wt : {1, 15})
                quirk += !k->mvOrderedWeights.empty() && k->mvOrderedWeights.back() >= wt;
        }
        // ---- single mutators
        for (int j = 0; j < 12; ++j) {
            KF* a = w.kfs[rng() % w.kfs.size()];
            KF* b = w.kfs[rng() % w.kfs.size()];
            switch (j % 3) {
                case 0: a->AddConnection(b, 10 + j); lm.AddConnection(a->mnId, b->mnId, 10 + j); break;
                case 1: a->EraseConnection(b); lm.EraseConnection(a->mnId, b->mnId); break;
                default: a->UpdateBestCovisibles(); lm.UpdateBestCovisibles(a->mnId);
            }
            bad += compare(lm, w, "mutators");
            ++steps;
        }
        // ---- the load-map loop (System.cc:188-191), in mnId order and in a shuffled one
        for (int pass = 0; pass < 2; ++pass) {
            std::vector<KF*> order = w.kfs;
            if (pass) std::shuffle(order.begin(), order.end(), rng);
            std::vector<uint64_t> ids;
            for (KF* k : order) {
                if (pass) {
                    k->mbFirstConnection = true;
                    lm.SetFirstConnection(k->mnId, true);
                }
                k->UpdateConnections();
                ids.push_back(k->mnId);
            }
            lm.UpdateConnections(ids);
            bad += compare(lm, w, "load-map loop");
            ++steps;
        }
        std::printf("COVIS DONE steps=%d keyframes=%d inversions=%d quirk=%d resorted=%d bad=%d\n", steps, nkf,
                    inversions, quirk, resorted, bad);
        return bad ? 1 : 0;
    } catch (const std::exception& e) {
        std::printf("ERROR %s\n", e.what());
        return 2;
    }
}
