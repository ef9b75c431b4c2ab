// orbfe_fuse.hip — ORBmatcher::Fuse (ORBmatcher.cc:828-978, the SE3 form of
// LocalMapping::SearchInNeighbors) and Fuse(pKF, Scw, ...) (980-1103, the Sim3 form of
// LoopClosing::SearchAndFuse) as one batched device search.
//
// Everything both overloads compute up to bestIdx / bestDist reads immutable data only (the
// point's position, normal, distance bounds and descriptor; the keyframe's pose, keypoints,
// descriptors and mvuRight), so the search of every (keyframe, point) pair runs at once and the
// host applies the Replace / AddObservation branch afterwards, walking the points in order
// (include/orbfe_orbslam.hpp ORBmatcher::Fuse).  No fixed point, no greedy rounds.
//
//   grid_kernel          (orbfe_grid.hip) KeyFrame::mGrid, the Frame grid, of every keyframe of
//                        the batch in one launch, one workgroup per keyframe
//   fuse_search_kernel   one wave per (keyframe, point): projection, KeyFrame::IsInImage,
//                        distance / viewing-angle tests, MapPoint::PredictScale,
//                        KeyFrame::GetFeaturesInArea (features_in_area_wave), the level and
//                        chi-square filters and the first-wins minimum Hamming distance
#include <hip/hip_runtime.h>

#include "../../include/orbfe.h"
#include "orbfe_device.hpp"

namespace orbfe {

constexpr int kFuseKfPerLaunch = 40;  // poses carried by one launch's kernel arguments

struct FuseArgs {
    const orbfe_keypoint* keys;  // keyframe kf at keys + kf * keys_pitch (keypoints)
    long long keys_pitch;
    const uint8_t* desc;         // desc + kf * desc_pitch (bytes, a multiple of 16)
    long long desc_pitch;
    const float* ur;             // ur + kf * kp_cap, or NULL: monocular (all -1)
    int kp_cap;                  // slab stride of ur and citems (>= 1)
    int kp_max;                  // keypoints a keyframe can hold: n_kp is clipped to it
    const int* n_kp;
    float minx, maxx, miny, maxy, gwi, ghi;
    const int* cstart;           // grid_kernel's outputs, one CSR per keyframe
    const int* citems;
    int n_mp;
    const float* xyz;
    const float* normal;
    const float* mind;           // mfMinDistance
    const float* maxd;           // mfMaxDistance
    const uint4* mdesc;
    const uint8_t* skip;         // [kf][n_mp] or NULL
    float fx, fy, cx, cy, bf;
    float log_scale, th;
    int nlevels;
    float scale[kMaxLevels];     // mvScaleFactors
    float inv_sigma2[kMaxLevels];  // mvInvLevelSigma2
    int* status;
    int* best_idx;               // [kf][n_mp]
    int* best_dist;              // [kf][n_mp] or NULL
    int kf0;                     // first keyframe of this launch
    float T[kFuseKfPerLaunch][12];  // Tcw of keyframes kf0 + blockIdx.y
    float ow[kFuseKfPerLaunch][3];  // camera centres (host, double accumulation)
};

__device__ __forceinline__ DevFrame fuse_frame(const FuseArgs& a, int kf) {
    return DevFrame{a.keys + kf * a.keys_pitch,
                    reinterpret_cast<const uint4*>(a.desc + kf * a.desc_pitch),
                    a.ur ? a.ur + (size_t)kf * a.kp_cap : nullptr,
                    min(max(a.n_kp[kf], 0), a.kp_max),
                    a.minx, a.maxx, a.miny, a.maxy, a.gwi, a.ghi,
                    a.cstart + (size_t)kf * (kGridCells + 1),
                    a.citems + (size_t)kf * a.kp_cap};
}

// One wave per (keyframe, point).  kSim3: the loop-closing overload, no chi-square test.
template <bool kSim3>
__global__ __launch_bounds__(256) void fuse_search_kernel(FuseArgs a) {
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= a.n_mp) return;
    const int kl = blockIdx.y, kf = a.kf0 + kl;
    const size_t o = (size_t)kf * a.n_mp + i;
    // every per-pair input is read up front and feeds the unconditional arithmetic below
    const bool sk = a.skip && a.skip[o];
    const float P[3] = {a.xyz[3 * i], a.xyz[3 * i + 1], a.xyz[3 * i + 2]};
    const float nv[3] = {a.normal[3 * i], a.normal[3 * i + 1], a.normal[3 * i + 2]};
    const float maxd = a.maxd[i], mind = a.mind[i];
    float pc[3];
    pose_apply(a.T[kl], P, pc);
    const float invz = 1.0f / pc[2];
    const float x = pc[0] * invz, y = pc[1] * invz;
    const float u = a.fx * x + a.cx, v = a.fy * y + a.cy;
    const float ur = u - a.bf * invz;
    const float po0 = P[0] - a.ow[kl][0], po1 = P[1] - a.ow[kl][1], po2 = P[2] - a.ow[kl][2];
    const float dist = (float)sqrt((double)po0 * po0 + (double)po1 * po1 + (double)po2 * po2);
    const double dot = (double)po0 * nv[0] + (double)po1 * nv[1] + (double)po2 * nv[2];
    const float dmax = kMaxDistInvariance * maxd, dmin = kMinDistInvariance * mind;
    // KeyFrame::IsInImage (KeyFrame.cc:1352): strict upper bounds
    const bool ok = !sk && !(pc[2] < 0.0f) && u >= a.minx && u < a.maxx && v >= a.miny &&
                    v < a.maxy && !(dist < dmin || dist > dmax) && !(dot < 0.5 * (double)dist);
    unsigned long long key = 256ull << 32;  // (distance, rank): strict <, bestDist starts at 256
    int kidx = -1;
    if (ok) {
        const int lvl = predict_level(maxd, dist, a.log_scale);
        if (level_in_pyramid(lvl, a.nlevels, a.status)) {
            const DevFrame F = fuse_frame(a, kf);
            const float radius = a.th * a.scale[lvl];
            const uint4 q0 = a.mdesc[2 * i], q1 = a.mdesc[2 * i + 1];
            // KeyFrame::GetFeaturesInArea(u, v, radius) has no level filter (KeyFrame.cc:1311);
            // the loop's own filters keep the survivors in the reference's order
            features_in_area_wave(
                F, u, v, radius, -1, -1,
                [&](int idx) {
                    const orbfe_keypoint kp = F.k[idx];
                    if (kp.octave < lvl - 1 || kp.octave > lvl) return false;
                    if (kSim3) return true;
                    const float inv = a.inv_sigma2[max(kp.octave, 0)];
                    const float kr = F.ur ? F.ur[idx] : -1.f;
                    const float ex = u - kp.x, ey = v - kp.y;
                    if (kr >= 0) {  // stereo reprojection error
                        const float er = ur - kr;
                        const float e2 = ex * ex + ey * ey + er * er;
                        return !((double)(e2 * inv) > 7.8);
                    }
                    const float e2 = ex * ex + ey * ey;
                    return !((double)(e2 * inv) > 5.99);
                },
                [&](int idx, int rank) {
                    const uint4* d = F.desc + 2 * (size_t)idx;
                    const unsigned long long c =
                        ((unsigned long long)hamming256(q0, q1, d[0], d[1]) << 32) | (unsigned)rank;
                    if (c < key) {
                        key = c;
                        kidx = idx;
                    }
                });
        }
    }
    wave_first_min(key, kidx);
    if ((threadIdx.x & 63) == 0) {
        const int bd = (int)(key >> 32);
        a.best_idx[o] = bd <= kThLow ? kidx : -1;
        if (a.best_dist) a.best_dist[o] = bd;
    }
}

}  // namespace orbfe

using namespace orbfe;

namespace {
// The grids of all n_kf keyframes in one launch, then the search: one launch per
// kFuseKfPerLaunch keyframes (their poses travel as kernel arguments).  a's device pointers and
// scalars are filled by the caller; asynchronous on the matcher's stream.
int fuse_launch(orbfe_matcher* m, FuseArgs& a, int n_kf, const float* tcw, int mode) {
    int st;
    if ((st = m->fu_cs.ensure((size_t)n_kf * (kGridCells + 1) * sizeof(int)))) return st;
    if ((st = m->fu_ci.ensure((size_t)n_kf * a.kp_cap * sizeof(int)))) return st;
    a.cstart = m->fu_cs.as<int>();
    a.citems = m->fu_ci.as<int>();
    hipLaunchKernelGGL(grid_kernel, dim3(n_kf), dim3(kGridBlock), 0, m->stream, a.keys,
                       a.keys_pitch, a.n_kp, a.kp_max, a.minx, a.miny, a.gwi, a.ghi,
                       m->fu_cs.as<int>(), m->fu_ci.as<int>(), a.kp_cap);
    for (int k0 = 0; k0 < n_kf; k0 += kFuseKfPerLaunch) {
        const int nk = std::min(kFuseKfPerLaunch, n_kf - k0);
        a.kf0 = k0;
        for (int k = 0; k < nk; ++k) {
            std::memcpy(a.T[k], tcw + 12 * (size_t)(k0 + k), 12 * sizeof(float));
            camera_center(a.T[k], a.ow[k]);
        }
        const dim3 grid((a.n_mp + 3) / 4, nk);
        if (mode == ORBFE_FUSE_SIM3)
            hipLaunchKernelGGL(fuse_search_kernel<true>, grid, dim3(256), 0, m->stream, a);
        else
            hipLaunchKernelGGL(fuse_search_kernel<false>, grid, dim3(256), 0, m->stream, a);
    }
    ORBFE_HIP(hipGetLastError());
    return ORBFE_OK;
}
}  // namespace

extern "C" {

int orbfe_fuse_search(orbfe_matcher* m, const orbfe_frame_view* kf, const float* tcw,
                      const orbfe_camera* cam, float log_scale_factor,
                      const float* inv_level_sigma2, int n_mp, const float* mp_xyz,
                      const float* mp_normal, const float* mp_min_dist,
                      const float* mp_max_dist, const uint8_t* mp_desc, const uint8_t* skip,
                      float th, int mode, int32_t* best_idx, int32_t* best_dist,
                      int32_t* n_found) {
    if (!m || !frame_ok(kf) || !tcw || !cam || !inv_level_sigma2 || !n_found || n_mp < 0 ||
        (mode != ORBFE_FUSE_SE3 && mode != ORBFE_FUSE_SIM3) ||
        (n_mp && (!mp_xyz || !mp_normal || !mp_min_dist || !mp_max_dist || !mp_desc || !best_idx)))
        return ORBFE_ERR_ARG;
    if (kf->nlevels > kMaxLevels) return ORBFE_ERR_UNSUPPORTED;
    *n_found = 0;
    if (n_mp == 0) return ORBFE_OK;
    return guarded(m, [&]() {
        int st;
        const int n = kf->n;
        const int32_t head[4] = {n, 0, 0, 0};  // {keypoint count, status}
        if ((st = m->up(m->scal, head, sizeof(head)))) return st;
        if ((st = m->up(m->fa_k, kf->keys_un, (size_t)n * sizeof(orbfe_keypoint)))) return st;
        if ((st = m->up(m->fa_d, kf->desc, (size_t)n * 32))) return st;
        if (kf->u_right && (st = m->up(m->fa_ur, kf->u_right, (size_t)n * sizeof(float)))) return st;
        if ((st = m->up(m->m_f0, mp_xyz, (size_t)n_mp * 12))) return st;
        if ((st = m->up(m->m_f1, mp_normal, (size_t)n_mp * 12))) return st;
        if ((st = m->up(m->m_f2, mp_min_dist, (size_t)n_mp * 4))) return st;
        if ((st = m->up(m->m_f3, mp_max_dist, (size_t)n_mp * 4))) return st;
        if ((st = m->up(m->m_d, mp_desc, (size_t)n_mp * 32))) return st;
        if (skip && (st = m->up(m->m_u0, skip, (size_t)n_mp))) return st;
        if ((st = m->s1.ensure((size_t)n_mp * sizeof(int)))) return st;
        if ((st = m->s2.ensure((size_t)n_mp * sizeof(int)))) return st;
        if ((st = m->flush())) return st;
        FuseArgs a{};
        a.keys = m->fa_k.as<orbfe_keypoint>();
        a.desc = m->fa_d.as<uint8_t>();
        a.ur = kf->u_right ? m->fa_ur.as<float>() : nullptr;
        a.kp_cap = std::max(n, 1);
        a.kp_max = n;
        a.n_kp = m->scal.as<int>();
        a.minx = kf->min_x;
        a.maxx = kf->max_x;
        a.miny = kf->min_y;
        a.maxy = kf->max_y;
        a.gwi = kf->grid_w_inv;
        a.ghi = kf->grid_h_inv;
        a.n_mp = n_mp;
        a.xyz = m->m_f0.as<float>();
        a.normal = m->m_f1.as<float>();
        a.mind = m->m_f2.as<float>();
        a.maxd = m->m_f3.as<float>();
        a.mdesc = m->m_d.as<uint4>();
        a.skip = skip ? m->m_u0.as<uint8_t>() : nullptr;
        a.fx = cam->fx;
        a.fy = cam->fy;
        a.cx = cam->cx;
        a.cy = cam->cy;
        a.bf = cam->bf;
        a.log_scale = log_scale_factor;
        a.th = th;
        a.nlevels = kf->nlevels;
        std::memcpy(a.scale, kf->scale_factors, (size_t)kf->nlevels * sizeof(float));
        std::memcpy(a.inv_sigma2, inv_level_sigma2, (size_t)kf->nlevels * sizeof(float));
        a.status = m->scal.as<int>() + 1;
        a.best_idx = m->s1.as<int>();
        a.best_dist = m->s2.as<int>();
        if ((st = fuse_launch(m, a, 1, tcw, mode))) return st;
        std::vector<int32_t> bd;
        if (!best_dist) bd.resize(n_mp);
        int status = 0;
        if ((st = m->down(best_idx, m->s1, (size_t)n_mp * 4))) return st;
        if ((st = m->down(best_dist ? best_dist : bd.data(), m->s2, (size_t)n_mp * 4))) return st;
        if ((st = m->down_ptr(&status, m->scal.as<int>() + 1, sizeof(int)))) return st;
        if ((st = m->sync())) return st;
        int nf = 0;
        for (int i = 0; i < n_mp; ++i) nf += best_idx[i] >= 0;
        *n_found = nf;
        return status;
    });
}

int orbfe_fuse_search_batch_device(orbfe_matcher* m, int n_kf, const orbfe_keypoint* d_keys,
                                   size_t keys_pitch, const uint8_t* d_desc, size_t desc_pitch,
                                   const float* d_u_right, int kp_cap, const int32_t* d_n,
                                   const float* tcw, const orbfe_camera* cam, float min_x,
                                   float max_x, float min_y, float max_y,
                                   const float* scale_factors, const float* inv_level_sigma2,
                                   int nlevels, float log_scale_factor, int n_mp,
                                   const float* d_xyz, const float* d_normal,
                                   const float* d_min_dist, const float* d_max_dist,
                                   const uint8_t* d_mp_desc, const uint8_t* d_skip, float th,
                                   int mode, int32_t* d_best_idx, int32_t* d_best_dist,
                                   int32_t* d_status) {
    if (!m || n_kf < 0 || n_mp < 0 || kp_cap < 0 || nlevels < 1 || !cam || !scale_factors ||
        !inv_level_sigma2 || !d_status || (mode != ORBFE_FUSE_SE3 && mode != ORBFE_FUSE_SIM3) ||
        (n_kf && (!d_n || !tcw || (kp_cap && (!d_keys || !d_desc)))) ||
        (n_kf && n_mp && (!d_xyz || !d_normal || !d_min_dist || !d_max_dist || !d_mp_desc ||
                          !d_best_idx)))
        return ORBFE_ERR_ARG;
    if ((desc_pitch & 15) ||
        (n_kf > 1 && (keys_pitch < (size_t)kp_cap || desc_pitch < (size_t)kp_cap * 32)))
        return ORBFE_ERR_ARG;
    if (nlevels > kMaxLevels) return ORBFE_ERR_UNSUPPORTED;
    return guarded(m, [&]() {
        ORBFE_HIP(hipMemsetAsync(d_status, 0, sizeof(int32_t), m->stream));
        if (n_kf == 0 || n_mp == 0) return ORBFE_OK;
        FuseArgs a{};
        a.keys = d_keys;
        a.keys_pitch = (long long)keys_pitch;
        a.desc = d_desc;
        a.desc_pitch = (long long)desc_pitch;
        a.ur = d_u_right;
        a.kp_cap = std::max(kp_cap, 1);
        a.kp_max = kp_cap;
        a.n_kp = d_n;
        a.minx = min_x;
        a.maxx = max_x;
        a.miny = min_y;
        a.maxy = max_y;
        a.gwi = (float)kGridCols / (max_x - min_x);  // mfGridElementWidthInv (Frame.cc:212-213)
        a.ghi = (float)kGridRows / (max_y - min_y);
        a.n_mp = n_mp;
        a.xyz = d_xyz;
        a.normal = d_normal;
        a.mind = d_min_dist;
        a.maxd = d_max_dist;
        a.mdesc = reinterpret_cast<const uint4*>(d_mp_desc);
        a.skip = d_skip;
        a.fx = cam->fx;
        a.fy = cam->fy;
        a.cx = cam->cx;
        a.cy = cam->cy;
        a.bf = cam->bf;
        a.log_scale = log_scale_factor;
        a.th = th;
        a.nlevels = nlevels;
        std::memcpy(a.scale, scale_factors, (size_t)nlevels * sizeof(float));
        std::memcpy(a.inv_sigma2, inv_level_sigma2, (size_t)nlevels * sizeof(float));
        a.status = d_status;
        a.best_idx = d_best_idx;
        a.best_dist = d_best_dist;
        return fuse_launch(m, a, n_kf, tcw, mode);
    });
}

}  // extern "C"
