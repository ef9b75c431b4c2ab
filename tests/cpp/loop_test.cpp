// The C++ adapter's loop-closing matchers (include/orbfe_orbslam.hpp) on a case dumped by
// tests/test_gpu_loop_cpp.py (tests/loop_cases.py dump_case): SearchByProjection(pKF, Scw, ...)
// with Scw un-normalised, SearchBySim3 with s12, R12, t12 as LoopClosing holds them (the
// adapter evaluates lines 1122-1124) and SearchByBoW(pKF1, pKF2).  Prints each call's return
// value and its vpMatched / vpMatches12; the Python side compares them with the restatements.
//
// Case file (little-endian): float cam[6]; FRAME kf; int32 n_mp, th; float log_scale, scw[12];
// xyz, normal (n_mp x 3), min_dist, max_dist, descriptors (n_mp); uint8 bad[n_mp]; int32
// ids[n_mp], matched0[kf.n]; FRAME kf1, kf2; POINTS pts1, pts2; float T1w[12], T2w[12], R12[9],
// t12[3], s12, th, log1, log2; int32 matches12[kf1.n], n_idx, (id, idx)[n_idx]; then per BoW
// side: int32 n; descriptors; float angle[n]; uint8 ok[n]; int32 nn, nfeat, node_ids[nn],
// node_off[nn + 1], feat[nfeat].
//   FRAME: int32 n, nlevels; float min_x, max_x, min_y, max_y, scale[nlevels]; keys, descriptors
//   POINTS (n = the frame's): int32 ids; uint8 bad; float xyz (x 3), min_dist, max_dist; descriptors
#include <cstdio>
#include <cstdlib>
#include <map>
#include <vector>

#include "../../include/orbfe_orbslam.hpp"

template <class T>
static std::vector<T> rd(FILE* f, size_t n) {
    std::vector<T> v(n);
    if (n && std::fread(v.data(), sizeof(T), n, f) != n) {
        std::fprintf(stderr, "loop_test: short case file\n");
        std::exit(2);
    }
    return v;
}

static orbfe::FrameData rd_frame(FILE* f) {
    const std::vector<int32_t> h = rd<int32_t>(f, 2);
    const std::vector<float> b = rd<float>(f, 4);
    orbfe::FrameData F;
    F.min_x = b[0];
    F.max_x = b[1];
    F.min_y = b[2];
    F.max_y = b[3];
    F.scale_factors = rd<float>(f, h[1]);
    F.keys_un = rd<orbfe_keypoint>(f, h[0]);
    F.descriptors = rd<uint8_t>(f, (size_t)h[0] * 32);
    return F;
}

struct Points {
    std::vector<int32_t> ids;
    std::vector<uint8_t> bad, desc;
    std::vector<float> xyz, mind, maxd;
    orbfe::KeyFramePoints view() const {
        orbfe::KeyFramePoints p;
        p.ids = ids.data();
        p.bad = bad.data();
        p.xyz = xyz.data();
        p.min_dist = mind.data();
        p.max_dist = maxd.data();
        p.desc = desc.data();
        return p;
    }
};

static Points rd_points(FILE* f, size_t n) {
    Points p;
    p.ids = rd<int32_t>(f, n);
    p.bad = rd<uint8_t>(f, n);
    p.xyz = rd<float>(f, 3 * n);
    p.mind = rd<float>(f, n);
    p.maxd = rd<float>(f, n);
    p.desc = rd<uint8_t>(f, 32 * n);
    return p;
}

struct BowSide {
    orbfe::FrameData F;
    Points P;
    std::vector<int32_t> node_ids, node_off, feat;
    orbfe::FeatureVectorView fv() const {
        return orbfe::FeatureVectorView{node_ids.data(), node_off.data(), feat.data(),
                                        (int)node_ids.size()};
    }
};

static BowSide rd_bow_side(FILE* f) {
    BowSide s;
    const int n = rd<int32_t>(f, 1)[0];
    s.F.descriptors = rd<uint8_t>(f, (size_t)n * 32);
    const std::vector<float> angle = rd<float>(f, n);
    const std::vector<uint8_t> ok = rd<uint8_t>(f, n);
    s.F.keys_un.assign(n, orbfe_keypoint{});
    s.P.ids.resize(n);
    s.P.bad.assign(n, 0);
    for (int i = 0; i < n; ++i) {
        s.F.keys_un[i].angle = angle[i];
        s.P.ids[i] = ok[i] ? 1000 + i : -1;
    }
    const std::vector<int32_t> h = rd<int32_t>(f, 2);
    s.node_ids = rd<int32_t>(f, h[0]);
    s.node_off = rd<int32_t>(f, h[0] + 1);
    s.feat = rd<int32_t>(f, h[1]);
    return s;
}

static void print(const char* name, int n, const std::vector<int>& v) {
    std::printf("%s n=%d\n%s_OUT", name, n, name);
    for (int x : v) std::printf(" %d", x);
    std::printf("\n");
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    const std::vector<float> cs = rd<float>(f, 6);
    const orbfe_camera cam{cs[0], cs[1], cs[2], cs[3], cs[4], cs[5]};
    // SearchByProjection(pKF, Scw, ...)
    const orbfe::FrameData KF = rd_frame(f);
    const std::vector<int32_t> h = rd<int32_t>(f, 2);
    const int n_mp = h[0], th = h[1];
    const float log_scale = rd<float>(f, 1)[0];
    const std::vector<float> scw_v = rd<float>(f, 12);
    orbfe::Sim3 scw;
    for (int i = 0; i < 12; ++i) scw.m[i] = scw_v[i];
    const std::vector<float> xyz = rd<float>(f, (size_t)n_mp * 3), nrm = rd<float>(f, (size_t)n_mp * 3);
    const std::vector<float> mind = rd<float>(f, n_mp), maxd = rd<float>(f, n_mp);
    const std::vector<uint8_t> desc = rd<uint8_t>(f, (size_t)n_mp * 32);
    const std::vector<uint8_t> bad = rd<uint8_t>(f, n_mp);
    const std::vector<int32_t> ids = rd<int32_t>(f, n_mp);
    std::vector<int> matched = rd<int32_t>(f, KF.keys_un.size());
    // SearchBySim3
    const orbfe::FrameData KF1 = rd_frame(f), KF2 = rd_frame(f);
    const Points P1 = rd_points(f, KF1.keys_un.size()), P2 = rd_points(f, KF2.keys_un.size());
    const std::vector<float> T1w = rd<float>(f, 12), T2w = rd<float>(f, 12), R12 = rd<float>(f, 9),
                             t12 = rd<float>(f, 3), sc = rd<float>(f, 4);
    std::vector<int> matches12 = rd<int32_t>(f, KF1.keys_un.size());
    const int n_idx = rd<int32_t>(f, 1)[0];
    const std::vector<int32_t> pairs = rd<int32_t>(f, (size_t)n_idx * 2);
    std::map<int, int> index_in_kf2;
    for (int i = 0; i < n_idx; ++i) index_in_kf2[pairs[2 * i]] = pairs[2 * i + 1];
    // SearchByBoW(pKF1, pKF2)
    const BowSide B1 = rd_bow_side(f), B2 = rd_bow_side(f);
    std::fclose(f);

    try {
        orbfe::ORBmatcher matcher(0.75f, true);
        orbfe::FusePoints pts;
        pts.n = n_mp;
        pts.xyz = xyz.data();
        pts.normal = nrm.data();
        pts.min_dist = mind.data();
        pts.max_dist = maxd.data();
        pts.desc = desc.data();
        pts.skip = bad.data();  // isBad(); the adapter adds spAlreadyFound
        const int n_sbp = matcher.SearchByProjection(KF, scw, cam, log_scale, pts, ids.data(),
                                                     matched, th);
        print("SBP", n_sbp, matched);
        const int n_sim3 = matcher.SearchBySim3(
            KF1, P1.view(), T1w.data(), sc[2], KF2, P2.view(), T2w.data(), sc[3], cam, matches12,
            sc[0], R12.data(), t12.data(), sc[1], [&](int id) {
                const auto it = index_in_kf2.find(id);
                return it == index_in_kf2.end() ? -1 : it->second;
            });
        print("SIM3", n_sim3, matches12);
        std::vector<int> bow12;
        const int n_bow = matcher.SearchByBoW(B1.F, B1.P.view(), B1.fv(), B2.F, B2.P.view(),
                                              B2.fv(), bow12);
        print("BOW", n_bow, bow12);
    } catch (const orbfe::Error& e) {
        std::printf("LOOP FAIL %s\n", e.what());
        return 1;
    }
    std::printf("LOOP DONE\n");
    return 0;
}
