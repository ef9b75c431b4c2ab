// The C++ adapter's ORBmatcher::SearchForTriangulation (include/orbfe_orbslam.hpp) on a case
// dumped by tests/test_gpu_triangulation_cpp.py (triangulation_cases.dump_case): the epipole from
// the pose (ORBmatcher.cc:667-673), the device search and the compaction into vMatchedPairs.
// Prints, for block_matched2 = 0 and 1, nmatches and the pair list; the Python side compares both
// with the restatement.
//
// Case file (little-endian): int32 n1, n2, nn1, nn2, tot1, tot2, nlevels, check_ori, only_stereo,
// stereo; float fx, fy, cx, cy, R2w[9], t2w[3], Cw[3], F12[9], scale[nlevels], sigma2[nlevels];
// then per keyframe: keys, descriptors, u_right (if stereo), uint8 has_mp, int32 node ids
// (nn), node offsets (nn + 1), features (tot).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../include/orbfe_orbslam.hpp"

template <class T>
static std::vector<T> rd(FILE* f, size_t n) {
    std::vector<T> v(n);
    if (n && std::fread(v.data(), sizeof(T), n, f) != n) {
        std::fprintf(stderr, "triangulation_test: short case file\n");
        std::exit(2);
    }
    return v;
}

struct Side {
    orbfe::FrameData frame;
    std::vector<uint8_t> mp;
    std::vector<int32_t> ids, off, feat;
};

static void read_side(FILE* f, Side& s, int n, int nn, int tot, int stereo,
                      const std::vector<float>& scale) {
    s.frame.keys_un = rd<orbfe_keypoint>(f, n);
    s.frame.descriptors = rd<uint8_t>(f, (size_t)n * 32);
    if (stereo) s.frame.u_right = rd<float>(f, n);
    s.frame.min_x = 0;
    s.frame.max_x = 640;
    s.frame.min_y = 0;
    s.frame.max_y = 480;
    s.frame.scale_factors = scale;
    s.mp = rd<uint8_t>(f, n);
    s.ids = rd<int32_t>(f, nn);
    s.off = rd<int32_t>(f, (size_t)nn + 1);
    s.feat = rd<int32_t>(f, tot);
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    const std::vector<int32_t> h = rd<int32_t>(f, 10);
    const int nlevels = h[6], check_ori = h[7], only_stereo = h[8], stereo = h[9];
    const std::vector<float> g = rd<float>(f, 4 + 9 + 3 + 3 + 9);
    const std::vector<float> scale = rd<float>(f, nlevels);
    const std::vector<float> sigma2 = rd<float>(f, nlevels);
    Side s1, s2;
    read_side(f, s1, h[0], h[2], h[4], stereo, scale);
    read_side(f, s2, h[1], h[3], h[5], stereo, scale);
    std::fclose(f);

    orbfe::KeyFrameData K1, K2;
    K1.frame = &s1.frame;
    K1.feat_vec = orbfe::FeatureVectorView{s1.ids.data(), s1.off.data(), s1.feat.data(), h[2]};
    K1.has_map_point = s1.mp.data();
    K1.Ow = &g[16];
    K2.frame = &s2.frame;
    K2.feat_vec = orbfe::FeatureVectorView{s2.ids.data(), s2.off.data(), s2.feat.data(), h[3]};
    K2.has_map_point = s2.mp.data();
    K2.Rcw = &g[4];
    K2.tcw = &g[13];
    K2.fx = g[0];
    K2.fy = g[1];
    K2.cx = g[2];
    K2.cy = g[3];
    K2.level_sigma2 = sigma2.data();
    const float* F12 = &g[19];

    try {
        orbfe::ORBmatcher matcher(0.6f, check_ori != 0);
        for (int block = 0; block < 2; ++block) {
            std::vector<std::pair<size_t, size_t>> pairs;
            // the default argument is the reference as written: call it that way for block 0
            const int n = block ? matcher.SearchForTriangulation(K1, K2, F12, pairs, only_stereo != 0, true)
                                : matcher.SearchForTriangulation(K1, K2, F12, pairs, only_stereo != 0);
            std::printf("BLOCK %d n=%d\n", block, n);
            for (const auto& p : pairs) std::printf("P %zu %zu\n", p.first, p.second);
        }
    } catch (const orbfe::Error& e) {
        std::fprintf(stderr, "triangulation_test: %s\n", e.what());
        return 1;
    }
    std::printf("TRIANGULATION DONE\n");
    return 0;
}
