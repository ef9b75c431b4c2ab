// orbfe_triangulate.hip — ORBmatcher::SearchForTriangulation (ORBmatcher.cc:660-826) with
// CheckDistEpipolarLine (140-157), over P (keyframe 1, keyframe 2) pairs at once:
// LocalMapping::CreateNewMapPoints matches the new keyframe against every covisible neighbour
// (LocalMapping.cc:207-268), and the host form is P = 1.  Keyframes are "slots" in the layout
// orbfe_bow_transform_batch_device writes (see BowMatchArgs in orbfe_bow.hip) plus, per slot, the
// undistorted keypoints, mvuRight and the map-point flags.
//
// The parallel form rests on the same fact as SearchByBoW's: DBoW2 lists a feature under exactly
// one node, so vbMatched2 couples only the keyframe-1 features of one common node.  A wave runs
// one node's loop (698-779) in the reference's order; nodes run in parallel.  The winner of one
// keyframe-1 feature is taken over the node's keyframe-2 features that are unmatched, hold no
// MapPoint, are stereo under bOnlyStereo, lie within TH_LOW and pass the epipole (746-752) and
// epipolar-line (754) tests: the smallest distance, LAST in node order on ties (`dist > bestDist`
// at 741 lets an equal distance replace the best).  The geometric tests do not depend on the
// loop's state and a candidate that fails them never lowers bestDist, so the reduction
// min (distance << 16 | 65535 - rank) over the passing candidates is exactly the loop's result.
//
// vbMatched2 (680) is read at 728 and never written in the reference, so as written no keyframe-2
// feature is ever blocked.  block_matched2 = 1 builds the evident intent
// (vbMatched2[bestIdx2] = true after 764, never released, not even when the orientation filter
// drops the match); block_matched2 = 0 is the literal source.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "../../include/orbfe.h"
#include "orbfe_device.hpp"

namespace orbfe {

struct TriArgs {
    int cap1, cap2;            // per-slot capacity of the keyframe-1 / keyframe-2 arrays
    const int* pair_1;         // [P] keyframe-1 slot per pair (NULL: slot 0)
    const int* pair_2;         // [P] keyframe-2 slot per pair (NULL: slot 0)
    // keyframe 1 (the new keyframe): pKF1->N, mFeatVec, GetMapPoint(i) != NULL, mDescriptors,
    // mvKeysUn, mvuRight (NULL: monocular, every entry -1)
    const int* n1;
    const int* nn1;
    const int* node_ids1;
    const int* node_off1;
    const int* feat1;
    const uint8_t* mp1;
    const uint4* desc1;
    const orbfe_keypoint* keys1;
    const float* ur1;
    // keyframe 2 (the neighbour)
    const int* n2;
    const int* nn2;
    const int* node_ids2;
    const int* node_off2;
    const int* feat2;
    const uint8_t* mp2;
    const uint4* desc2;
    const orbfe_keypoint* keys2;
    const float* ur2;
    const float* f12;          // [P][9] row-major F12
    const float* epipole;      // [P][2] ex, ey (667-673)
    int nlevels;
    float scale[kMaxLevels];   // pKF2->mvScaleFactors
    float sigma2[kMaxLevels];  // pKF2->mvLevelSigma2
    int only_stereo, check_ori, block;
    int* matches;              // [P][cap1] vMatches12
    int* bins;                 // [P][cap1] scratch: rotation bin of each match
    int* hist;                 // [P][32] rotation histogram
    int* nm;                   // [P] nmatches
    int* done;                 // [P] workgroups of the pair that finished the node loop
    int* status;               // ORBFE_ERR_UNSUPPORTED / ORBFE_ERR_ARG on bad input
};

__device__ __forceinline__ float readlane_f(float v, int l) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}

constexpr int kTriBlock = 256;    // 4 waves
constexpr int kTriNodeMax = 256;  // keyframe-2 features per node held in registers (4 per lane)

// Waves stride over keyframe 1's nodes (grid.y = pairs); lower_bound into keyframe 2's node ids
// finds the common node (694-792).  Lanes hold the node's keyframe-2 features (rank r = lane +
// 64 j, the order of f2it->second): descriptor, position, the two octave-dependent thresholds
// and the eligibility bits.  The node's keyframe-1 features are fetched 64 at a time — each lane
// also evaluates its feature's epipolar line (143-145) — and broadcast in order.
__global__ __launch_bounds__(kTriBlock) void tri_search_kernel(TriArgs a) {
    __shared__ float s_epi_th[kMaxLevels];   // 100 * mvScaleFactors[octave] (750)
    __shared__ double s_line_th[kMaxLevels]; // 3.84 * mvLevelSigma2[octave], in double (156)
    if (threadIdx.x < kMaxLevels) {
        const int l = threadIdx.x < a.nlevels ? threadIdx.x : 0;
        s_epi_th[threadIdx.x] = 100 * a.scale[l];
        s_line_th[threadIdx.x] = 3.84 * a.sigma2[l];
    }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int p = blockIdx.y;
    const int s1 = a.pair_1 ? a.pair_1[p] : 0, s2 = a.pair_2 ? a.pair_2[p] : 0;
    const int n1 = a.n1[s1], n2 = a.n2[s2], nn1 = a.nn1[s1], nn2 = a.nn2[s2];
    const size_t b1 = (size_t)s1 * a.cap1, b2 = (size_t)s2 * a.cap2;
    const int* node_ids1 = a.node_ids1 + b1;
    const int* node_off1 = a.node_off1 + (size_t)s1 * (a.cap1 + 1);
    const int* feat1 = a.feat1 + b1;
    const uint8_t* mp1 = a.mp1 + b1;
    const uint4* desc1 = a.desc1 + 2 * b1;
    const orbfe_keypoint* keys1 = a.keys1 + b1;
    const float* ur1 = a.ur1 ? a.ur1 + b1 : nullptr;
    const int* node_ids2 = a.node_ids2 + b2;
    const int* node_off2 = a.node_off2 + (size_t)s2 * (a.cap2 + 1);
    const int* feat2 = a.feat2 + b2;
    const uint8_t* mp2 = a.mp2 + b2;
    const uint4* desc2 = a.desc2 + 2 * b2;
    const orbfe_keypoint* keys2 = a.keys2 + b2;
    const float* ur2 = a.ur2 ? a.ur2 + b2 : nullptr;
    const float* F = a.f12 + 9 * (size_t)p;
    const float f00 = F[0], f01 = F[1], f02 = F[2], f10 = F[3], f11 = F[4], f12 = F[5],
                f20 = F[6], f21 = F[7], f22 = F[8];
    const float ex = a.epipole[2 * (size_t)p], ey = a.epipole[2 * (size_t)p + 1];
    int* matches = a.matches + (size_t)p * a.cap1;
    int* bins = a.bins + (size_t)p * a.cap1;
    int* hist = a.hist + p * 32;
    const bool bad = n1 < 0 || n1 > a.cap1 || n2 < 0 || n2 > a.cap2 || nn1 < 0 || nn1 > a.cap1 ||
                     nn2 < 0 || nn2 > a.cap2;
    if (bad && threadIdx.x == 0) atomicExch(a.status, ORBFE_ERR_ARG);
    const int nwaves = gridDim.x * (kTriBlock / 64);
    const int n_nodes = bad ? 0 : nn1;
    for (int na = blockIdx.x * (kTriBlock / 64) + (threadIdx.x >> 6); na < n_nodes; na += nwaves) {
        const int fb = bow_pair_of(node_ids2, nn2, node_ids1[na]);
        if (fb < 0) continue;
        const int y0 = node_off2[fb], ny = node_off2[fb + 1] - y0;
        const int x0 = node_off1[na], nx = node_off1[na + 1] - x0;
        if (y0 < 0 || ny < 0 || y0 + ny > a.cap2 || x0 < 0 || nx < 0 || x0 + nx > a.cap1) {
            if (lane == 0) atomicExch(a.status, ORBFE_ERR_ARG);
            continue;
        }
        if (ny > kTriNodeMax) {
            if (lane == 0) atomicExch(a.status, ORBFE_ERR_UNSUPPORTED);
            continue;
        }
        int i2[4];
        uint4 d0[4], d1[4];
        float x2[4], y2[4], eth[4];
        double lth[4];
        bool live[4], st2[4];
        bool arg_err = false;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int r = lane + 64 * j;
            i2[j] = -1;
            live[j] = false;
            st2[j] = false;
            d0[j] = d1[j] = make_uint4(0, 0, 0, 0);
            x2[j] = y2[j] = eth[j] = 0.f;
            lth[j] = 0.0;
            if (r < ny) {
                const int k = feat2[y0 + r];
                if (k < 0 || k >= n2) {
                    arg_err = true;
                    continue;
                }
                const orbfe_keypoint kp = keys2[k];
                if (kp.octave < 0 || kp.octave >= a.nlevels) {
                    arg_err = true;
                    continue;
                }
                i2[j] = k;
                st2[j] = ur2 && ur2[k] >= 0;                       // bStereo2 (731)
                live[j] = !mp2[k] && (!a.only_stereo || st2[j]);   // 728, 733-735
                d0[j] = desc2[2 * k];
                d1[j] = desc2[2 * k + 1];
                x2[j] = kp.x;
                y2[j] = kp.y;
                eth[j] = s_epi_th[kp.octave];
                lth[j] = s_line_th[kp.octave];
            }
        }
        if (arg_err) atomicExch(a.status, ORBFE_ERR_ARG);
        const int nj = (ny + 63) >> 6;  // candidate registers in use (wave-uniform)
        for (int xb = 0; xb < nx; xb += 64) {
            const int xl = xb + lane;
            int my_i1 = -1, my_st1 = 0;
            uint4 my0 = make_uint4(0, 0, 0, 0), my1 = my0;
            float my_a = 0.f, my_b = 0.f, my_c = 0.f, my_ang = 0.f;
            if (xl < nx) {
                const int k = feat1[x0 + xl];
                if (k < 0 || k >= n1) {
                    atomicExch(a.status, ORBFE_ERR_ARG);
                } else {
                    my_st1 = ur1 && ur1[k] >= 0;  // bStereo1 (708)
                    if (!mp1[k] && (!a.only_stereo || my_st1)) {  // 705-712
                        my_i1 = k;
                        my0 = desc1[2 * k];
                        my1 = desc1[2 * k + 1];
                        const orbfe_keypoint kp = keys1[k];
                        // l = x1' F12 = [a b c] (143-145)
                        my_a = kp.x * f00 + kp.y * f10 + f20;
                        my_b = kp.x * f01 + kp.y * f11 + f21;
                        my_c = kp.x * f02 + kp.y * f12 + f22;
                        my_ang = kp.angle;
                    }
                }
            }
            const int cnt = min(64, nx - xb);
            for (int t = 0; t < cnt; ++t) {
                // t is wave-uniform: v_readlane into scalar registers
                const int i1 = __builtin_amdgcn_readlane(my_i1, t);
                if (i1 < 0) continue;
                uint4 q0, q1;
                readlane_desc(my0, my1, t, q0, q1);
                const float la = readlane_f(my_a, t), lb = readlane_f(my_b, t),
                            lc = readlane_f(my_c, t);
                const bool st1 = __builtin_amdgcn_readlane(my_st1, t) != 0;
                const float ang1 = readlane_f(my_ang, t);
                const float den = la * la + lb * lb;  // 149
                uint32_t key = 0xffffffffu;
                if (den != 0) {  // 151-152: every candidate fails the line test otherwise
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        if (j < nj && live[j]) {
                            const int dist = hamming256(q0, q1, d0[j], d1[j]);
                            bool ok = dist <= kThLow;  // 741
                            if (!st1 && !st2[j]) {     // 746-752
                                const float distex = ex - x2[j];
                                const float distey = ey - y2[j];
                                if (distex * distex + distey * distey < eth[j]) ok = false;
                            }
                            const float num = la * x2[j] + lb * y2[j] + lc;  // 147
                            const float dsqr = num * num / den;             // 154
                            if (!((double)dsqr < lth[j])) ok = false;       // 156
                            if (ok)
                                key = min(key, ((uint32_t)dist << 16) |
                                                   (uint32_t)(0xffff - (lane + 64 * j)));
                        }
                    }
                }
                key = __ockl_wfred_min_u32(key);  // DPP wave reduction: min distance, max rank
                if (key == 0xffffffffu) continue;
                const int brank = 0xffff - (int)(key & 0xffff);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (lane + 64 * j == brank) {
                        if (a.block) live[j] = false;  // vbMatched2[bestIdx2] (H13)
                        matches[i1] = i2[j];           // 764
                        if (a.check_ori) {             // 767-777
                            const int bin = rot_bin(ang1, keys2[i2[j]].angle);
                            bins[i1] = bin;
                            // angles outside [0, 360) can leave the histogram, where the
                            // reference's assert (775) fires: the match is dropped
                            if (bin >= 0 && bin < kHistLen) atomicAdd(&hist[bin], 1);
                            else atomicExch(a.status, ORBFE_ERR_UNSUPPORTED);
                        }
                        atomicAdd(&a.nm[p], 1);
                    }
                }
            }
        }
    }
    if (!a.check_ori) return;
    // the pair's last workgroup to finish runs the orientation filter
    if (!last_workgroup(&a.done[p])) return;
    ori_filter(matches, bins, hist, &a.nm[p], a.cap1);  // 794-813, shared with SearchByBoW
}

}  // namespace orbfe

using namespace orbfe;

namespace {
int tri_launch(orbfe_matcher* m, const TriArgs& a, int n_pairs, int gx) {
    // vMatches12 = -1 (681) per keyframe-1 feature, nmatches = 0 (679)
    hipLaunchKernelGGL(pair_init_kernel, dim3(n_pairs), dim3(256), 0, m->stream, a.matches, a.cap1,
                       a.hist, a.nm, a.done, a.status);
    hipLaunchKernelGGL(tri_search_kernel, dim3(gx, n_pairs), dim3(kTriBlock), 0, m->stream, a);
    ORBFE_HIP(hipGetLastError());
    return ORBFE_OK;
}
}  // namespace

extern "C" {

int orbfe_search_for_triangulation(orbfe_matcher* m, int check_ori, int block_matched2,
                                   int only_stereo, const orbfe_frame_view* kf1,
                                   const uint8_t* has_mp1, int nn1, const int32_t* node_ids1,
                                   const int32_t* node_off1, const int32_t* feat1,
                                   const orbfe_frame_view* kf2, const uint8_t* has_mp2, int nn2,
                                   const int32_t* node_ids2, const int32_t* node_off2,
                                   const int32_t* feat2, const float* f12, const float* epipole,
                                   const float* level_sigma2, int32_t* matches12,
                                   int32_t* nmatches) {
    if (!m || !frame_ok(kf1) || !frame_ok(kf2) || nn1 < 0 || nn2 < 0 || !f12 || !epipole ||
        !level_sigma2 || !nmatches || (kf1->n && (!has_mp1 || !matches12)) ||
        (kf2->n && !has_mp2) || (nn1 && (!node_ids1 || !node_off1 || !feat1)) ||
        (nn2 && (!node_ids2 || !node_off2 || !feat2)))
        return ORBFE_ERR_ARG;
    if (kf2->nlevels > kMaxLevels) return ORBFE_ERR_UNSUPPORTED;
    const int n1 = kf1->n, n2 = kf2->n;
    if (!fv_ok(nn1, node_off1, feat1, n1) || !fv_ok(nn2, node_off2, feat2, n2))
        return ORBFE_ERR_ARG;
    const int tot1 = nn1 ? node_off1[nn1] : 0, tot2 = nn2 ? node_off2[nn2] : 0;
    return guarded(m, [&]() {
        int st;
        for (int i = 0; i < n1; ++i) matches12[i] = -1;  // vMatches12 (681)
        *nmatches = 0;
        if (!nn1 || !nn2 || !n1 || !n2) return ORBFE_OK;
        // slot 0 of each side; the caps bound every offset and index (validated above)
        const int cap1 = std::max(n1, nn1), cap2 = std::max(n2, nn2);
        const int cnt[4] = {n1, n2, nn1, nn2};
        float geo[11];
        std::memcpy(geo, f12, 9 * sizeof(float));
        geo[9] = epipole[0];
        geo[10] = epipole[1];
        if ((st = m->up(m->fa_k, kf1->keys_un, (size_t)n1 * sizeof(orbfe_keypoint)))) return st;
        if ((st = m->up(m->fa_d, kf1->desc, (size_t)n1 * 32))) return st;
        if (kf1->u_right && (st = m->up(m->fa_ur, kf1->u_right, (size_t)n1 * 4))) return st;
        if ((st = m->up(m->m_u0, has_mp1, n1))) return st;
        if ((st = m->up(m->fa_cs, node_ids1, (size_t)nn1 * 4))) return st;
        if ((st = m->up(m->fa_ci, node_off1, (size_t)(nn1 + 1) * 4))) return st;
        if ((st = m->up(m->fa_co, feat1, (size_t)tot1 * 4))) return st;
        if ((st = m->up(m->fb_k, kf2->keys_un, (size_t)n2 * sizeof(orbfe_keypoint)))) return st;
        if ((st = m->up(m->fb_d, kf2->desc, (size_t)n2 * 32))) return st;
        if (kf2->u_right && (st = m->up(m->fb_ur, kf2->u_right, (size_t)n2 * 4))) return st;
        if ((st = m->up(m->m_u1, has_mp2, n2))) return st;
        if ((st = m->up(m->fb_cs, node_ids2, (size_t)nn2 * 4))) return st;
        if ((st = m->up(m->fb_ci, node_off2, (size_t)(nn2 + 1) * 4))) return st;
        if ((st = m->up(m->fb_co, feat2, (size_t)tot2 * 4))) return st;
        if ((st = m->up(m->nq, cnt, sizeof(cnt)))) return st;
        if ((st = m->up(m->m_f0, geo, sizeof(geo)))) return st;
        if ((st = m->s1.ensure((size_t)cap1 * 4))) return st;  // matches
        if ((st = m->s2.ensure((size_t)cap1 * 4))) return st;  // bins
        if ((st = m->g_hist.ensure(64 * sizeof(int)))) return st;
        if ((st = m->scal.ensure(16))) return st;
        if ((st = m->flush())) return st;
        TriArgs a{};
        a.cap1 = cap1;
        a.cap2 = cap2;
        a.n1 = m->nq.as<int>();
        a.n2 = m->nq.as<int>() + 1;
        a.nn1 = m->nq.as<int>() + 2;
        a.nn2 = m->nq.as<int>() + 3;
        a.node_ids1 = m->fa_cs.as<int>();
        a.node_off1 = m->fa_ci.as<int>();
        a.feat1 = m->fa_co.as<int>();
        a.mp1 = m->m_u0.as<uint8_t>();
        a.desc1 = m->fa_d.as<uint4>();
        a.keys1 = m->fa_k.as<orbfe_keypoint>();
        a.ur1 = kf1->u_right ? m->fa_ur.as<float>() : nullptr;
        a.node_ids2 = m->fb_cs.as<int>();
        a.node_off2 = m->fb_ci.as<int>();
        a.feat2 = m->fb_co.as<int>();
        a.mp2 = m->m_u1.as<uint8_t>();
        a.desc2 = m->fb_d.as<uint4>();
        a.keys2 = m->fb_k.as<orbfe_keypoint>();
        a.ur2 = kf2->u_right ? m->fb_ur.as<float>() : nullptr;
        a.f12 = m->m_f0.as<float>();
        a.epipole = m->m_f0.as<float>() + 9;
        a.nlevels = kf2->nlevels;
        std::memcpy(a.scale, kf2->scale_factors, (size_t)kf2->nlevels * sizeof(float));
        std::memcpy(a.sigma2, level_sigma2, (size_t)kf2->nlevels * sizeof(float));
        a.only_stereo = only_stereo != 0;
        a.check_ori = check_ori != 0;
        a.block = block_matched2 != 0;
        a.matches = m->s1.as<int>();
        a.bins = m->s2.as<int>();
        a.hist = m->g_hist.as<int>();
        a.done = m->g_hist.as<int>() + 32;
        a.nm = m->scal.as<int>();
        a.status = m->scal.as<int>() + 1;
        if ((st = tri_launch(m, a, 1, std::min((nn1 + 3) / 4, 256)))) return st;
        int res[2] = {0, 0};
        if ((st = m->down(matches12, m->s1, (size_t)n1 * 4))) return st;
        if ((st = m->down(res, m->scal, sizeof(res)))) return st;
        if ((st = m->sync())) return st;
        *nmatches = res[0];
        return res[1];  // ORBFE_ERR_UNSUPPORTED: a node held more than 256 keyframe-2 features
    });
}

int orbfe_search_for_triangulation_batch_device(
    orbfe_matcher* m, int check_ori, int block_matched2, int only_stereo, int cap,
    const orbfe_keypoint* d_keys, const uint8_t* d_desc, const float* d_u_right,
    const uint8_t* d_has_mp, const int32_t* d_n, const int32_t* d_nn, const int32_t* d_node_ids,
    const int32_t* d_node_off, const int32_t* d_feat, int n_pairs, const int32_t* d_pair_1,
    const int32_t* d_pair_2, const float* d_f12, const float* d_epipole,
    const float* scale_factors, const float* level_sigma2, int nlevels, int32_t* d_matches12,
    int32_t* d_nmatches, int32_t* d_status) {
    if (!m || n_pairs < 0 || n_pairs > 65535 || cap < 1 || nlevels < 1 || !d_keys || !d_desc ||
        !d_has_mp || !d_n || !d_nn || !d_node_ids || !d_node_off || !d_feat || !d_pair_1 ||
        !d_pair_2 || !d_f12 || !d_epipole || !scale_factors || !level_sigma2 || !d_matches12 ||
        !d_nmatches || !d_status)
        return ORBFE_ERR_ARG;
    if (nlevels > kMaxLevels) return ORBFE_ERR_UNSUPPORTED;
    return guarded(m, [&]() {
        int st;
        if (n_pairs == 0) {
            ORBFE_HIP(hipMemsetAsync(d_status, 0, sizeof(int32_t), m->stream));
            return ORBFE_OK;
        }
        if ((st = m->s2.ensure((size_t)n_pairs * cap * 4))) return st;
        if ((st = m->g_hist.ensure((size_t)n_pairs * 33 * sizeof(int)))) return st;
        TriArgs a{};
        a.cap1 = a.cap2 = cap;
        a.pair_1 = d_pair_1;
        a.pair_2 = d_pair_2;
        a.n1 = a.n2 = d_n;
        a.nn1 = a.nn2 = d_nn;
        a.node_ids1 = a.node_ids2 = d_node_ids;
        a.node_off1 = a.node_off2 = d_node_off;
        a.feat1 = a.feat2 = d_feat;
        a.mp1 = a.mp2 = d_has_mp;
        a.desc1 = a.desc2 = reinterpret_cast<const uint4*>(d_desc);
        a.keys1 = a.keys2 = d_keys;
        a.ur1 = a.ur2 = d_u_right;
        a.f12 = d_f12;
        a.epipole = d_epipole;
        a.nlevels = nlevels;
        std::memcpy(a.scale, scale_factors, (size_t)nlevels * sizeof(float));
        std::memcpy(a.sigma2, level_sigma2, (size_t)nlevels * sizeof(float));
        a.only_stereo = only_stereo != 0;
        a.check_ori = check_ori != 0;
        a.block = block_matched2 != 0;
        a.matches = d_matches12;
        a.bins = m->s2.as<int>();
        a.hist = m->g_hist.as<int>();
        a.done = m->g_hist.as<int>() + (size_t)n_pairs * 32;
        a.nm = d_nmatches;
        a.status = d_status;
        // as SearchByBoW's batch: enough workgroups per pair to fill the chip
        const int gx = std::max(1, std::min((cap + 3) / 4, (1024 + n_pairs - 1) / n_pairs));
        return tri_launch(m, a, n_pairs, std::min(gx, 32));
    });
}

}  // extern "C"
