// refresh_test — the C++ adapter's MapPoint refresh (orbfe::LocalMap, include/orbfe_orbslam.hpp)
// against MapPoint::UpdateNormalAndDepth (MapPoint.cc:571-619), ComputeDistinctiveDescriptors
// (:483-548), EraseObservation with its mpRefKF rule (:352-378) and the map-point loop of
// LocalMapping::ProcessNewKeyFrame (LocalMapping.cc:140-161) written out over heap-allocated
// stand-in structs with a real std::map<KF*, size_t>: the addresses are whatever the allocator
// gives, so "order_key = the pointer" is what is tested.  cv::Mat arithmetic is spelled out in the
// readings of DESIGN.md H29, one helper each.
//
//   refresh_test <seed>   a random map; every point refreshed by list; single erases on reference
//                         keyframes; a keyframe set bad; the keyframe form; a new keyframe through
//                         ProcessNewKeyFrame; Replace's descriptor-only path.  After every step
//                         every point's mpRefKF, normal, distances and descriptor are compared.
#include <dlfcn.h>

#include <algorithm>
#include <array>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iterator>
#include <map>
#include <random>
#include <vector>

#include "../../include/orbfe_orbslam.hpp"

namespace {

// ---- the three readings (H29)
float recip(double s) { return (float)(1.0 / s); }                  // Mat / double
float axpy(float acc, float d, float a) {                           // Mat + Mat * a
    volatile float t = d * a;
    return acc + t;
}
float mean(float acc, int n) { return acc * recip((double)n); }     // Mat / int
double norm3(const float d[3]) { return std::sqrt(((double)d[0] * d[0] + (double)d[1] * d[1]) + (double)d[2] * d[2]); }

struct KF;
std::vector<float> g_scale;

struct MP {
    uint64_t mnId = 0;
    bool mbBad = false;
    std::map<KF*, size_t> mObservations;
    KF* mpRefKF = nullptr;
    int nObs = 0;
    float mWorldPos[3] = {0, 0, 0}, mNormalVector[3] = {9, 9, 9}, mfMinDistance = -7, mfMaxDistance = -9;
    std::array<uint8_t, 32> mDescriptor{};
    bool isBad() const { return mbBad; }
    bool IsInKeyFrame(KF* pKF) const { return mObservations.count(pKF) != 0; }
    void AddObservation(KF* pKF, size_t idx);
    void EraseObservation(KF* pKF);
    void SetBadFlag();
    void UpdateNormalAndDepth();
    void ComputeDistinctiveDescriptors();
};

struct KF {
    uint64_t mnId = 0;
    bool mbBad = false;
    std::vector<MP*> mvpMapPoints;
    std::vector<int> octave;
    std::vector<float> mvuRight;
    std::vector<std::array<uint8_t, 32>> mDescriptors;
    float Ow[3] = {0, 0, 0};
    bool isBad() const { return mbBad; }
};

void MP::AddObservation(KF* pKF, size_t idx) {  // MapPoint.cc:339-350
    if (mObservations.count(pKF)) return;
    mObservations[pKF] = idx;
    if (pKF->mvuRight[idx] >= 0) nObs += 2;
    else nObs++;
}

void MP::SetBadFlag() {  // :392-409
    std::map<KF*, size_t> obs;
    mbBad = true;
    obs = mObservations;
    mObservations.clear();
    for (auto& e : obs) e.first->mvpMapPoints[e.second] = nullptr;
}

void MP::EraseObservation(KF* pKF) {  // :352-378
    bool bBad = false;
    if (mObservations.count(pKF)) {
        const int idx = (int)mObservations[pKF];
        if (pKF->mvuRight[idx] >= 0) nObs -= 2;
        else nObs--;
        mObservations.erase(pKF);
        if (mpRefKF == pKF)  // begin() of an empty map: the mirror stores NULL (H29)
            mpRefKF = mObservations.empty() ? nullptr : mObservations.begin()->first;
        if (nObs <= 2) bBad = true;
    }
    if (bBad) SetBadFlag();
}

int hamming(const std::array<uint8_t, 32>& a, const std::array<uint8_t, 32>& b) {
    int d = 0;
    for (int i = 0; i < 32; ++i) d += __builtin_popcount((unsigned)(a[i] ^ b[i]));
    return d;
}

void MP::ComputeDistinctiveDescriptors() {  // :483-548
    if (mbBad) return;
    std::map<KF*, size_t> observations = mObservations;
    if (observations.empty()) return;
    std::vector<std::array<uint8_t, 32>> vDescriptors;
    for (auto mit = observations.begin(); mit != observations.end(); mit++) {
        KF* pKF = mit->first;
        if (!pKF->isBad()) vDescriptors.push_back(pKF->mDescriptors[mit->second]);
    }
    if (vDescriptors.empty()) return;
    const size_t N = vDescriptors.size();
    std::vector<std::vector<float>> Distances(N, std::vector<float>(N));
    for (size_t i = 0; i < N; i++) {
        Distances[i][i] = 0;
        for (size_t j = i + 1; j < N; j++) {
            const int distij = hamming(vDescriptors[i], vDescriptors[j]);
            Distances[i][j] = distij;
            Distances[j][i] = distij;
        }
    }
    int BestMedian = INT_MAX;
    int BestIdx = 0;
    for (size_t i = 0; i < N; i++) {
        std::vector<int> vDists(Distances[i].begin(), Distances[i].end());
        std::sort(vDists.begin(), vDists.end());
        const int median = vDists[0.5 * (N - 1)];
        if (median < BestMedian) {
            BestMedian = median;
            BestIdx = i;
        }
    }
    mDescriptor = vDescriptors[BestIdx];
}

void MP::UpdateNormalAndDepth() {  // :571-619
    if (mbBad) return;
    std::map<KF*, size_t> observations = mObservations;
    KF* pRefKF = mpRefKF;
    if (observations.empty()) return;
    float normal[3] = {0, 0, 0};
    int n = 0;
    for (auto mit = observations.begin(); mit != observations.end(); mit++) {
        KF* pKF = mit->first;
        float normali[3];
        for (int k = 0; k < 3; ++k) normali[k] = mWorldPos[k] - pKF->Ow[k];
        const float a = recip(norm3(normali));
        for (int k = 0; k < 3; ++k) normal[k] = axpy(normal[k], normali[k], a);
        n++;
    }
    if (!pRefKF) return;
    float PC[3];
    for (int k = 0; k < 3; ++k) PC[k] = mWorldPos[k] - pRefKF->Ow[k];
    const float dist = (float)norm3(PC);
    const int level = pRefKF->octave[observations[pRefKF]];
    const float levelScaleFactor = g_scale[level];
    const int nLevels = (int)g_scale.size();
    mfMaxDistance = dist * levelScaleFactor;
    mfMinDistance = mfMaxDistance / g_scale[nLevels - 1];
    for (int k = 0; k < 3; ++k) mNormalVector[k] = mean(normal[k], n);
}

// LocalMapping.cc:140-161
void ProcessNewKeyFrame(KF* mpCurrentKeyFrame, std::vector<MP*>& mlpRecentAddedMapPoints) {
    const std::vector<MP*> vpMapPointMatches = mpCurrentKeyFrame->mvpMapPoints;
    for (size_t i = 0; i < vpMapPointMatches.size(); i++) {
        MP* pMP = vpMapPointMatches[i];
        if (pMP) {
            if (!pMP->isBad()) {
                if (!pMP->IsInKeyFrame(mpCurrentKeyFrame)) {
                    pMP->AddObservation(mpCurrentKeyFrame, i);
                    pMP->UpdateNormalAndDepth();
                    pMP->ComputeDistinctiveDescriptors();
                } else {
                    mlpRecentAddedMapPoints.push_back(pMP);
                }
            }
        }
    }
}

// device memory without the HIP headers: the runtime is loaded with liborbfe.so
using MallocFn = int (*)(void**, size_t);
using MemcpyFn = int (*)(void*, const void*, size_t, int);
MallocFn hip_malloc;
MemcpyFn hip_memcpy;

#define REQUIRE(c)                                                       \
    do {                                                                 \
        if (!(c)) {                                                      \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);   \
            std::exit(1);                                                \
        }                                                                \
    } while (0)

struct World {
    std::vector<KF*> kfs;
    std::vector<MP*> mps;
    orbfe::LocalMap lm;
    orbfe_map_point_arrays arr{};
    size_t cap = 0;

    void upload_xyz() {
        std::vector<float> x(3 * cap, 0.f);
        for (MP* p : mps) std::memcpy(&x[3 * lm.MapPointSlot(p->mnId)], p->mWorldPos, 12);
        REQUIRE(hip_memcpy(arr.xyz, x.data(), x.size() * 4, 1) == 0);
    }
    void compare(const char* step) {
        std::vector<float> nrm(3 * cap), mn(cap), mx(cap);
        std::vector<uint8_t> ds(32 * cap);
        REQUIRE(hip_memcpy(nrm.data(), arr.normal, nrm.size() * 4, 2) == 0);
        REQUIRE(hip_memcpy(mn.data(), arr.min_dist, mn.size() * 4, 2) == 0);
        REQUIRE(hip_memcpy(mx.data(), arr.max_dist, mx.size() * 4, 2) == 0);
        REQUIRE(hip_memcpy(ds.data(), arr.desc, ds.size(), 2) == 0);
        for (MP* p : mps) {
            const size_t s = (size_t)lm.MapPointSlot(p->mnId);
            const uint64_t ref = lm.GetReferenceKeyFrame(p->mnId);
            const bool ok = std::memcmp(&nrm[3 * s], p->mNormalVector, 12) == 0 &&
                            std::memcmp(&mn[s], &p->mfMinDistance, 4) == 0 &&
                            std::memcmp(&mx[s], &p->mfMaxDistance, 4) == 0 &&
                            std::memcmp(&ds[32 * s], p->mDescriptor.data(), 32) == 0 &&
                            ref == (p->mpRefKF ? p->mpRefKF->mnId : orbfe::LocalMap::kNone) &&
                            lm.MapPointIsBad(p->mnId) == p->mbBad && lm.Observations(p->mnId) == p->nObs;
            if (!ok) {
                std::printf("FAILED after %s: point %llu\n", step, (unsigned long long)p->mnId);
                std::exit(1);
            }
        }
    }
};

}  // namespace

int main(int argc, char** argv) {
    const unsigned seed = argc > 1 ? (unsigned)std::atoi(argv[1]) : 1;
    std::mt19937 rng(seed);
    auto uni = [&](float a, float b) { return std::uniform_real_distribution<float>(a, b)(rng); };
    auto pick = [&](int n) { return (int)(rng() % (unsigned)n); };
    World w;
    hip_malloc = (MallocFn)dlsym(RTLD_DEFAULT, "hipMalloc");
    hip_memcpy = (MemcpyFn)dlsym(RTLD_DEFAULT, "hipMemcpy");
    REQUIRE(hip_malloc && hip_memcpy);
    const int K = 12, S = 40, P = 150;
    w.cap = P + 8;
    REQUIRE(hip_malloc((void**)&w.arr.xyz, 12 * w.cap) == 0 && hip_malloc((void**)&w.arr.normal, 12 * w.cap) == 0 &&
            hip_malloc((void**)&w.arr.min_dist, 4 * w.cap) == 0 && hip_malloc((void**)&w.arr.max_dist, 4 * w.cap) == 0 &&
            hip_malloc((void**)&w.arr.desc, 32 * w.cap) == 0);
    for (int i = 0; i < 8; ++i) g_scale.push_back(std::pow(1.2f, (float)i));
    w.lm.SetScaleFactors(g_scale);
    for (int j = 0; j < P; ++j) {
        MP* p = new MP;
        p->mnId = 1000 + j;
        for (float& x : p->mWorldPos) x = uni(-8, 8);
        p->mWorldPos[2] += 12;
        p->mDescriptor.fill(0xA5);
        w.mps.push_back(p);
        w.lm.NewMapPoint(p->mnId);
    }
    auto new_kf = [&](uint64_t id, const std::vector<MP*>& row) {
        KF* k = new KF;
        k->mnId = id;
        k->mvpMapPoints = row;
        std::vector<uint64_t> ids;
        for (MP* p : row) ids.push_back(p ? p->mnId : orbfe::LocalMap::kNone);
        for (size_t i = 0; i < row.size(); ++i) {
            k->octave.push_back(pick(8));
            k->mvuRight.push_back(pick(3) == 0 ? 1.f : -1.f);
            std::array<uint8_t, 32> d;
            for (uint8_t& b : d) b = (uint8_t)(pick(4) == 0 ? rng() : 0x3c);  // near neighbours: median ties
            k->mDescriptors.push_back(d);
        }
        for (float& x : k->Ow) x = uni(-3, 3);
        w.kfs.push_back(k);
        w.lm.NewKeyFrame(id, (uint64_t)(uintptr_t)k, ids);
        w.lm.SetKeyFrameFeatures(id, std::vector<int32_t>(k->octave.begin(), k->octave.end()), k->mvuRight, {}, 40.f);
        w.lm.SetDescriptors(id, k->mDescriptors[0].data(), row.size());
        w.lm.SetCameraCenter(id, k->Ow);
        return k;
    };
    for (int i = 0; i < K; ++i) {
        std::vector<MP*> row(S, nullptr);
        for (int s = 0; s < S; ++s)
            if (pick(5)) row[s] = w.mps[pick(P)];
        KF* k = new_kf(10 + i, row);
        for (int s = 0; s < S; ++s)
            if (row[s] && !row[s]->IsInKeyFrame(k)) {
                row[s]->AddObservation(k, s);
                w.lm.AddObservation(row[s]->mnId, k->mnId, s);
            }
    }
    std::vector<uint64_t> all;
    for (MP* p : w.mps) {
        all.push_back(p->mnId);
        if (!p->mObservations.empty() && pick(8)) {
            auto it = p->mObservations.begin();
            std::advance(it, pick((int)p->mObservations.size()));
            p->mpRefKF = it->first;
            w.lm.SetReferenceKeyFrame(p->mnId, p->mpRefKF->mnId);
        }
    }
    w.upload_xyz();
    {   // the sentinels the literal structs start with
        std::vector<float> nine(3 * w.cap, 9.f), m7(w.cap, -7.f), m9(w.cap, -9.f);
        std::vector<uint8_t> a5(32 * w.cap, 0xA5);
        REQUIRE(hip_memcpy(w.arr.normal, nine.data(), nine.size() * 4, 1) == 0);
        REQUIRE(hip_memcpy(w.arr.min_dist, m7.data(), m7.size() * 4, 1) == 0);
        REQUIRE(hip_memcpy(w.arr.max_dist, m9.data(), m9.size() * 4, 1) == 0);
        REQUIRE(hip_memcpy(w.arr.desc, a5.data(), a5.size(), 1) == 0);
    }
    w.compare("building");
    // every point by list
    for (MP* p : w.mps) {
        p->UpdateNormalAndDepth();
        p->ComputeDistinctiveDescriptors();
    }
    w.lm.RefreshPoints(all, 3, w.arr);
    w.compare("RefreshPoints");
    // single erases on reference keyframes (MapPoint.cc:367-368), some of which set the point bad
    int moved = 0, went = 0;
    for (MP* p : w.mps) {
        if (!p->mpRefKF || p->mbBad || pick(3)) continue;
        KF* k = p->mpRefKF;
        bool bad = false;
        p->EraseObservation(k);
        w.lm.EraseObservation(p->mnId, k->mnId, &bad);
        REQUIRE(bad == p->mbBad);
        moved += p->mpRefKF != nullptr;
        went += bad;
    }
    w.compare("EraseObservation");
    // a bad keyframe: left out of the descriptor, counted for the normal
    w.kfs[3]->mbBad = true;
    w.lm.set_keyframe_bad(w.kfs[3]->mnId);
    for (MP* p : w.kfs[5]->mvpMapPoints)
        if (p) {
            p->UpdateNormalAndDepth();
            p->ComputeDistinctiveDescriptors();
        }
    w.lm.RefreshKeyFramePoints(w.kfs[5]->mnId, w.arr);
    w.compare("RefreshKeyFramePoints");
    // a new keyframe: points not yet observed, observed already (stereo points), held twice, bad
    std::vector<MP*> row(S, nullptr);
    for (int s = 0; s < S; ++s)
        if (pick(4)) row[s] = w.mps[pick(P)];
    row[S - 1] = row[0] ? row[0] : w.mps[0];
    KF* nk = new_kf(99, row);
    for (int s = 1; s < S; s += 7)
        if (row[s] && !row[s]->mbBad && !row[s]->IsInKeyFrame(nk)) {
            row[s]->AddObservation(nk, s);
            w.lm.AddObservation(row[s]->mnId, nk->mnId, s);
        }
    std::vector<MP*> recent;
    ProcessNewKeyFrame(nk, recent);
    const std::vector<uint64_t> got = w.lm.ProcessNewKeyFrame(nk->mnId, w.arr);
    REQUIRE(got.size() == recent.size());
    for (size_t i = 0; i < got.size(); ++i) REQUIRE(got[i] == recent[i]->mnId);
    w.compare("ProcessNewKeyFrame");
    // MapPoint::Replace's last line: the descriptor alone, of one point
    for (int t = 0; t < 10; ++t) {
        MP* p = w.mps[pick(P)];
        p->ComputeDistinctiveDescriptors();
        w.lm.ComputeDistinctiveDescriptors(p->mnId, w.arr);
    }
    w.compare("ComputeDistinctiveDescriptors");
    std::printf("refresh_test seed %u: ok (%d references moved, %d points went bad, %zu recent)\n", seed, moved,
                went, recent.size());
    return 0;
}
