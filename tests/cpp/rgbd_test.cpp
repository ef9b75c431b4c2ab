// The C++ adapter's RGB-D path (include/orbfe_orbslam.hpp) against the reference's loops written
// out literally in this program: ORBextractor::ComputeStereoFromRGBD against the lookup loop of
// Frame::ComputeStereoFromRGBD (Frame.cc:759-780) on the converted image, and
// ORBmatcher::ClosePoints against the std::sort of vector<pair<float, int>> and the nPoints walk of
// Tracking::UpdateLastFrame (Tracking.cc:1059-1111) with Frame::UnprojectStereo (Frame.cc:782-796)
// and the MapPoint constructor's distances (MapPoint.cc:298-305).  Every float compares on its
// bits.  The case is built here from a fixed generator: a 640 x 480 16-bit depth image quantised so
// that depths tie, 400 keypoints at fractional positions, undistorted twins moved off them.
// Prints "RGBD DONE" when everything agrees (run by tests/test_gpu_rgbd_cpp.py).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <utility>
#include <vector>

#include "../../include/orbfe_orbslam.hpp"

static uint32_t g_state = 12345u;
static uint32_t rnd() {
    g_state = g_state * 1664525u + 1013904223u;
    return g_state >> 8;
}
static float unit() { return (float)(rnd() & 0xffff) / 65536.0f; }

static int g_fail = 0;
static void expect_bits(const char* what, const std::vector<float>& a, const std::vector<float>& b) {
    if (a.size() != b.size() || (a.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(float)))) {
        std::printf("MISMATCH %s\n", what);
        g_fail = 1;
    }
}
template <class T>
static void expect_eq(const char* what, const T& a, const T& b) {
    if (!(a == b)) {
        std::printf("MISMATCH %s\n", what);
        g_fail = 1;
    }
}

struct Literal {
    std::vector<int> order;
    std::vector<uint8_t> create;
    std::vector<float> xyz, max_dist, min_dist;
    int n_total = 0, n_map = 0;
};

// The walk of Tracking.cc:1061-1111 (sorted = true) or 764-779 (sorted = false).
static Literal literal_close(bool sorted, const orbfe::FrameData& F, const std::vector<float>& mvDepth,
                             const orbfe_camera& cam, const float* Rwc, const float* Ow, float mThDepth) {
    Literal L;
    const int N = (int)F.keys_un.size();
    const float invfx = 1.0f / cam.fx, invfy = 1.0f / cam.fy;
    auto has_point = [&](int i) { return F.map_points[i] >= 0 && F.map_point_obs[i] >= 1; };
    for (int i = 0; i < N; i++) {  // 1256-1265
        if (mvDepth[i] > 0 && mvDepth[i] < mThDepth) {
            L.n_total++;
            if (has_point(i)) L.n_map++;
        }
    }
    std::vector<std::pair<float, int> > vDepthIdx;
    for (int i = 0; i < N; i++) {
        float z = mvDepth[i];
        if (z > 0) vDepthIdx.push_back(std::make_pair(z, i));
    }
    if (vDepthIdx.empty()) return L;
    if (sorted) std::sort(vDepthIdx.begin(), vDepthIdx.end());
    int nPoints = 0;
    for (size_t j = 0; j < vDepthIdx.size(); j++) {
        int i = vDepthIdx[j].second;
        bool bCreateNew = !sorted || !has_point(i);
        float P[3] = {0, 0, 0}, mx = 0, mn = 0;
        if (bCreateNew) {
            const float z = mvDepth[i];
            const float u = F.keys_un[i].x, v = F.keys_un[i].y;
            const float x = (u - cam.cx) * z * invfx;
            const float y = (v - cam.cy) * z * invfy;
            for (int r = 0; r < 3; r++)
                P[r] = ((Rwc[3 * r] * x + Rwc[3 * r + 1] * y) + Rwc[3 * r + 2] * z) + Ow[r];
            double s = 0;
            for (int r = 0; r < 3; r++) {
                const float d = P[r] - Ow[r];
                s += (double)d * d;
            }
            const float dist = (float)std::sqrt(s);
            mx = dist * F.scale_factors[F.keys_un[i].octave];
            mn = mx / F.scale_factors[F.scale_factors.size() - 1];
        }
        nPoints++;
        L.order.push_back(i);
        L.create.push_back(bCreateNew ? 1 : 0);
        L.xyz.insert(L.xyz.end(), P, P + 3);
        L.max_dist.push_back(mx);
        L.min_dist.push_back(mn);
        if (sorted && vDepthIdx[j].first > mThDepth && nPoints > 100) break;
    }
    return L;
}

int main() {
    const int W = 640, H = 480, N = 400;
    const float factor = 1.0f / 5000.0f, bf = 40.0f;
    std::vector<uint16_t> imDepth((size_t)W * H);
    for (auto& d : imDepth) d = (rnd() % 8 == 0) ? 0 : (uint16_t)(2000 + 500 * (rnd() % 60));
    orbfe::FrameData F;
    std::vector<orbfe_keypoint> mvKeys(N);
    for (int i = 0; i < N; i++) {
        orbfe_keypoint k{};
        k.x = unit() * (W - 1);
        k.y = unit() * (H - 1);
        k.octave = (int)(rnd() % 8);
        mvKeys[i] = k;
        k.x += unit() * 4 - 2;
        k.y += unit() * 4 - 2;
        F.keys_un.push_back(k);
        F.map_points.push_back(rnd() % 3 == 0 ? (int)i : -1);
        F.map_point_obs.push_back((int)(rnd() % 3));
    }
    for (int l = 0; l < 8; l++) F.scale_factors.push_back(l ? F.scale_factors[l - 1] * 1.2f : 1.0f);

    orbfe::ORBextractor ex(1000, 1.2f, 8, 20, 7, 0, W, H);
    // the literal lookup on the converted image
    std::vector<float> wantU(N, -1.f), wantD(N, -1.f);
    for (int i = 0; i < N; i++) {
        const float v = mvKeys[i].y, u = mvKeys[i].x;
        const float d = (float)imDepth[(size_t)(int)v * W + (int)u] * factor;
        if (d > 0) {
            wantD[i] = d;
            wantU[i] = F.keys_un[i].x - bf / d;
        }
    }
    std::vector<float> mvuRight, mvDepth;
    ex.ComputeStereoFromRGBD(imDepth.data(), ORBFE_DEPTH_U16, W, H, (size_t)W * 2, factor, mvKeys, F.keys_un,
                             bf, mvuRight, mvDepth);
    expect_bits("mvuRight (foreign pointer)", mvuRight, wantU);
    expect_bits("mvDepth (foreign pointer)", mvDepth, wantD);
    size_t step = 0;
    void* buf = ex.DepthBuffer(W, H, ORBFE_DEPTH_U16, &step);
    for (int y = 0; y < H; y++) std::memcpy((uint8_t*)buf + y * step, &imDepth[(size_t)y * W], (size_t)W * 2);
    ex.ComputeStereoFromRGBD(buf, ORBFE_DEPTH_U16, W, H, step, factor, mvKeys, F.keys_un, bf, mvuRight, mvDepth);
    expect_bits("mvuRight (depth buffer)", mvuRight, wantU);
    expect_bits("mvDepth (depth buffer)", mvDepth, wantD);
    int with_depth = 0;
    for (float d : mvDepth) with_depth += d > 0;
    std::printf("STEREO n=%d with_depth=%d\n", N, with_depth);

    orbfe_camera cam{517.3f, 516.5f, 318.6f, 255.3f, bf, bf / 517.3f};
    const float Rwc[9] = {0.36f, 0.48f, -0.8f, -0.8f, 0.6f, 0.0f, 0.48f, 0.64f, 0.6f};
    const float Ow[3] = {0.7f, -1.3f, 2.1f};
    orbfe::ORBmatcher matcher(0.9f, true, 0);
    // thresholds with more than and fewer than 100 depths inside, and one beyond every depth
    const float ths[3] = {4.05f, 1.25f, 100.0f};
    for (int t = 0; t < 4; t++) {
        const bool sorted = t < 3;
        const float th = ths[t % 3];
        const Literal want = literal_close(sorted, F, mvDepth, cam, Rwc, Ow, th);
        const orbfe::ClosePointsResult got =
            matcher.ClosePoints(sorted ? ORBFE_CLOSE_SORTED : ORBFE_CLOSE_ALL, F, mvDepth, cam, Rwc, Ow, th);
        expect_eq("order", got.order, want.order);
        expect_eq("create", got.create, want.create);
        expect_bits("xyz", got.xyz, want.xyz);
        expect_bits("max_dist", got.max_dist, want.max_dist);
        expect_bits("min_dist", got.min_dist, want.min_dist);
        expect_eq("n_total", got.n_total, want.n_total);
        expect_eq("n_map", got.n_map, want.n_map);
        expect_eq("octave flag", got.octave_out_of_pyramid, false);
        std::printf("CLOSE mode=%d th=%g visited=%zu n_total=%d n_map=%d\n", sorted ? 0 : 1, th,
                    got.order.size(), got.n_total, got.n_map);
    }
    if (g_fail) return 1;
    std::printf("RGBD DONE\n");
    return 0;
}
