// The C++ adapter's ORBmatcher::Fuse overloads (include/orbfe_orbslam.hpp) on a case dumped by
// tests/test_gpu_fuse_cpp.py: the device search plus the ordered walk, with callables that keep
// a small model of the keyframe's slots and the points' state (the tail of ORBmatcher.cc:955-974
// and 1085-1099) and record every call.  Prints, per overload, nFused and the call sequence; the
// Python side compares both with its own walk over the restatement's search.
//
// Case file (little-endian): int32 n_kp, stereo, n_mp, nlevels, n_ids; float min_x, max_x,
// min_y, max_y, cam[6], log_scale, th_se3, th_sim3, tcw[12], scw[12], scale[nlevels],
// inv_sigma2[nlevels]; keys, descriptors, u_right (n_kp); xyz, normal (n_mp x 3), min_dist,
// max_dist, descriptors (n_mp); int32 pid[n_mp], slot[n_kp], nobs[n_ids]; uint8 bad[n_ids],
// in_kf[n_ids].
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../include/orbfe_orbslam.hpp"

template <class T>
static std::vector<T> rd(FILE* f, size_t n) {
    std::vector<T> v(n);
    if (n && std::fread(v.data(), sizeof(T), n, f) != n) {
        std::fprintf(stderr, "fuse_test: short case file\n");
        std::exit(2);
    }
    return v;
}

struct Model {
    std::vector<int32_t> pid, slot, nobs;
    std::vector<uint8_t> bad, in_kf;
    bool skipped(int i) const { return bad[pid[i]] || in_kf[pid[i]]; }
    void replace(int old_id, int new_id) {  // MapPoint::Replace within this keyframe
        bad[old_id] = 1;
        for (size_t s = 0; s < slot.size(); ++s)
            if (slot[s] == old_id) {
                if (!in_kf[new_id]) {
                    slot[s] = new_id;
                    in_kf[new_id] = 1;
                } else {
                    slot[s] = -1;
                }
                in_kf[old_id] = 0;
                break;
            }
        nobs[new_id] += nobs[old_id];
    }
};

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    const std::vector<int32_t> h = rd<int32_t>(f, 5);
    const int n_kp = h[0], stereo = h[1], n_mp = h[2], nlevels = h[3], n_ids = h[4];
    const std::vector<float> s = rd<float>(f, 4 + 6 + 3 + 12 + 12);
    orbfe::FrameData KF;
    KF.min_x = s[0];
    KF.max_x = s[1];
    KF.min_y = s[2];
    KF.max_y = s[3];
    const orbfe_camera cam{s[4], s[5], s[6], s[7], s[8], s[9]};
    const float log_scale = s[10], th_se3 = s[11], th_sim3 = s[12];
    const float* tcw = &s[13];
    orbfe::Sim3 scw;
    for (int i = 0; i < 12; ++i) scw.m[i] = s[25 + i];
    KF.scale_factors = rd<float>(f, nlevels);
    const std::vector<float> inv_sigma2 = rd<float>(f, nlevels);
    KF.keys_un = rd<orbfe_keypoint>(f, n_kp);
    KF.descriptors = rd<uint8_t>(f, (size_t)n_kp * 32);
    KF.u_right = rd<float>(f, n_kp);
    if (!stereo) KF.u_right.clear();
    const std::vector<float> xyz = rd<float>(f, (size_t)n_mp * 3), nrm = rd<float>(f, (size_t)n_mp * 3);
    const std::vector<float> mind = rd<float>(f, n_mp), maxd = rd<float>(f, n_mp);
    const std::vector<uint8_t> desc = rd<uint8_t>(f, (size_t)n_mp * 32);
    Model start;
    start.pid = rd<int32_t>(f, n_mp);
    start.slot = rd<int32_t>(f, n_kp);
    start.nobs = rd<int32_t>(f, n_ids);
    start.bad = rd<uint8_t>(f, n_ids);
    start.in_kf = rd<uint8_t>(f, n_ids);
    std::fclose(f);

    try {
        orbfe::ORBmatcher matcher(0.6f, true);
        for (int sim3 = 0; sim3 < 2; ++sim3) {
            Model m = start;
            std::vector<uint8_t> skip(n_mp);
            for (int i = 0; i < n_mp; ++i) skip[i] = m.skipped(i);
            orbfe::FusePoints pts;
            pts.n = n_mp;
            pts.xyz = xyz.data();
            pts.normal = nrm.data();
            pts.min_dist = mind.data();
            pts.max_dist = maxd.data();
            pts.desc = desc.data();
            pts.skip = skip.data();
            std::vector<std::string> calls;
            auto skipped = [&](int i) { return m.skipped(i); };
            auto occupied = [&](int idx) { return m.slot[idx] >= 0; };
            auto on_occupied = [&](int i, int idx) {
                calls.push_back("O " + std::to_string(i) + " " + std::to_string(idx));
                const int p = m.pid[i], pin = m.slot[idx];
                if (m.bad[pin] || sim3) return;  // Sim3: vpReplacePoint[i] = pMPinKF, no state change
                if (m.nobs[pin] > m.nobs[p])
                    m.replace(p, pin);
                else
                    m.replace(pin, p);
            };
            auto on_empty = [&](int i, int idx) {
                calls.push_back("E " + std::to_string(i) + " " + std::to_string(idx));
                const int p = m.pid[i];
                m.nobs[p] += 1;
                m.in_kf[p] = 1;
                m.slot[idx] = p;
            };
            const int nFused =
                sim3 ? matcher.Fuse(KF, scw, cam, log_scale, pts, th_sim3, skipped, occupied,
                                    on_occupied, on_empty)
                     : matcher.Fuse(KF, tcw, cam, log_scale, inv_sigma2, pts, th_se3, skipped,
                                    occupied, on_occupied, on_empty);
            std::printf("MODE %s nFused=%d\n", sim3 ? "SIM3" : "SE3", nFused);
            for (const std::string& c : calls) std::printf("%s\n", c.c_str());
            std::printf("SLOTS");
            for (int v : m.slot) std::printf(" %d", v);
            std::printf("\n");
        }
    } catch (const orbfe::Error& e) {
        std::printf("FUSE FAIL %s\n", e.what());
        return 1;
    }
    std::printf("FUSE DONE\n");
    return 0;
}
