// orbfe_loop.hip — the matchers LoopClosing::ComputeSim3 calls on a loop candidate:
//
//   SearchByProjection(KeyFrame* pKF, cv::Mat Scw, vpPoints, vpMatched, int th)
//       (ORBmatcher.cc:293-406, LoopClosing.cc:376): projection, in-image, distance and viewing
//       tests and the predicted level per point (this overload's own forms of them around the
//       shared pieces of orbfe_grid.hip), then a greedy tail — a keypoint that held a point
//       before the call, or that an earlier point of the list took (378, 399), is blocked.
//       sbp_loop_cand_kernel
//       builds every point's candidates in parallel; orbfe_greedy.hip resolves the order
//       dependence (kGreedyMaxD, max_dist = TH_LOW, every acceptance blocks), driven by
//       sbp_search (orbfe_match_api.hip) like the other host forms.
//   SearchBySim3(pKF1, pKF2, vpMatches12, s12, R12, t12, th)
//       (ORBmatcher.cc:1105-1329, LoopClosing.cc:324): two independent projection searches
//       (KF1's points into KF2 and back) in one launch of sim3_search_kernel (grid.y = 2, a wave
//       per source feature), then sim3_agree_kernel keeps the pairs both directions chose.  No
//       greedy dependency, no rounds.
//   SearchByBoW(pKF1, pKF2, vpMatches12) (ORBmatcher.cc:525-658, LoopClosing.cc:266, once per
//       loop candidate): bow_search_kk_kernel, the per-node wave search of orbfe_bow.hip with
//       both sides keyframes; a host form (one pair) and a batch over keyframe slots.
#include <hip/hip_runtime.h>

#include "../../include/orbfe.h"
#include "orbfe_device.hpp"

namespace orbfe {

// ---------------------------------------------------------------------------------------------
// SearchByProjection(pKF, Scw, vpPoints, vpMatched, th) (ORBmatcher.cc:293-406)
struct SbpLoopArgs {
    DevFrame kf;
    int n;
    const uint8_t* skip;      // isBad() || spAlreadyFound.count(pMP) (320); NULL: none
    const float* xyz;
    const float* normal;
    const float* mind;        // mfMinDistance
    const float* maxd;        // mfMaxDistance
    const uint4* desc;
    float T[12];              // the normalised [Rcw|tcw] (302-305)
    float ow[3];              // -Rcw^T tcw (host, double accumulation)
    float fx, fy, cx, cy;
    float minx, maxx, miny, maxy;
    const float* scale;
    int nlevels;
    float log_scale, th;      // th = (float)(int th) (363)
    int* status;
    CandArgs c;               // kMode 2 uses kfix / ovf
};

// kMode: CandSink's (orbfe_grid.hip).  This overload's own choices (334-362): invz a float
// divide, x = X * invz before fx * x + cx, KeyFrame::IsInImage's strict upper bounds, dot <
// 0.5 * dist in double; the [lvl - 1, lvl] window sits in the keep filter, so the survivors of
// KeyFrame::GetFeaturesInArea(u, v, radius) (no level filter, KeyFrame.cc:1311) keep the
// reference's order.
template <int kMode>
__global__ __launch_bounds__(256) void sbp_loop_cand_kernel(SbpLoopArgs a) {
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);  // one wave per point of the list
    if (i >= a.n) return;
    const CandSink<kMode> sink{a.c, i};
    // every per-point input is read up front and feeds the unconditional arithmetic below
    const bool room = sink.room();
    const bool sk = a.skip && a.skip[i];
    const float P[3] = {a.xyz[3 * i], a.xyz[3 * i + 1], a.xyz[3 * i + 2]};
    const float nv[3] = {a.normal[3 * i], a.normal[3 * i + 1], a.normal[3 * i + 2]};
    const float maxd = a.maxd[i], mind = a.mind[i];
    if (!room) return;
    int n = 0;
    {
        float pc[3];
        pose_apply(a.T, P, pc);
        const float invz = 1.0f / pc[2];  // 1/p3Dc.at<float>(2): a float divide (334)
        const float x = pc[0] * invz, y = pc[1] * invz;
        const float u = a.fx * x + a.cx, v = a.fy * y + a.cy;
        const float po0 = P[0] - a.ow[0], po1 = P[1] - a.ow[1], po2 = P[2] - a.ow[2];
        const float dist = (float)sqrt((double)po0 * po0 + (double)po1 * po1 + (double)po2 * po2);
        const double dot = (double)po0 * nv[0] + (double)po1 * nv[1] + (double)po2 * nv[2];
        const float dmax = kMaxDistInvariance * maxd, dmin = kMinDistInvariance * mind;
        const bool ok = !sk && !(pc[2] < 0.0f) && u >= a.minx && u < a.maxx && v >= a.miny &&
                        v < a.maxy && !(dist < dmin || dist > dmax) && !(dot < 0.5 * (double)dist);
        if (ok) {
            const int lvl = predict_level(maxd, dist, a.log_scale);
            if (level_in_pyramid(lvl, a.nlevels, a.status)) {
                const float radius = a.th * a.scale[lvl];
                const uint4 q0 = a.desc[2 * i], q1 = a.desc[2 * i + 1];
                int2* out = sink.out();
                n = features_in_area_wave(
                    a.kf, u, v, radius, -1, -1,
                    [&](int i2) {  // 381-384
                        const int o = a.kf.k[i2].octave;
                        return !(o < lvl - 1 || o > lvl);
                    },
                    [&](int i2, int rank) {
                        sink.put(out, rank, i2, [&] {
                            const uint4* d = a.kf.desc + 2 * i2;
                            return hamming256(q0, q1, d[0], d[1]);
                        });
                    });
            }
        }
    }
    sink.finish(n);
}

// ---------------------------------------------------------------------------------------------
// SearchBySim3 (ORBmatcher.cc:1105-1329)
// One direction: the source keyframe's features (each with the map point it holds) projected
// into the target keyframe.
struct Sim3Side {
    DevFrame tgt;             // the target's keypoints, descriptors, image bounds and grid
    int n;                    // source features
    const uint8_t* search;    // point present, not bad, not already matched (1155-1159)
    const float* xyz;         // GetWorldPos() of the source's points
    const float* mind;        // mfMinDistance
    const float* maxd;        // mfMaxDistance
    const uint4* desc;        // the MapPoint's descriptor (1200)
    float Tsw[12];            // source camera from world
    float S[12];              // [sR|t]: source camera -> target camera (1122-1124)
    float log_scale;          // the target's mfLogScaleFactor
    int nlevels;              // the target's pyramid
    float scale[kMaxLevels];  // the target's mvScaleFactors
    int* vn;                  // out: vnMatch of the source, n entries
};
struct Sim3Args {
    Sim3Side s[2];            // [0]: KF1 -> KF2, [1]: KF2 -> KF1
    float fx, fy, cx, cy;     // pKF1's, in both directions (1108-1111)
    float th;
    int* status;
};

__global__ __launch_bounds__(256) void sim3_search_kernel(Sim3Args a) {
    const Sim3Side& s = a.s[blockIdx.y];
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);  // one wave per source feature
    if (i >= s.n) return;
    // every per-feature input is read up front and feeds the unconditional arithmetic below
    const bool live = s.search[i] != 0;
    const float P[3] = {s.xyz[3 * i], s.xyz[3 * i + 1], s.xyz[3 * i + 2]};
    const float maxd = s.maxd[i], mind = s.mind[i];
    float p1[3], p2[3];
    pose_apply(s.Tsw, P, p1);  // world -> source camera (1162)
    pose_apply(s.S, p1, p2);   // -> target camera (1163)
    const float invz = (float)(1.0 / (double)p2[2]);  // 1.0/p3Dc2.at<float>(2): double divide (1169)
    const float x = p2[0] * invz, y = p2[1] * invz;
    const float u = a.fx * x + a.cx, v = a.fy * y + a.cy;
    // cv::norm of the camera-frame vector, accumulated in double (1182)
    const float dist = (float)sqrt((double)p2[0] * p2[0] + (double)p2[1] * p2[1] + (double)p2[2] * p2[2]);
    const float dmax = kMaxDistInvariance * maxd, dmin = kMinDistInvariance * mind;
    const DevFrame& F = s.tgt;
    const bool ok = live && !(p2[2] < 0.0f) && u >= F.minx && u < F.maxx && v >= F.miny &&
                    v < F.maxy && !(dist < dmin || dist > dmax);
    // (distance, rank): strict <, bestDist starts at INT_MAX (1202); no key reaches 257 << 32
    unsigned long long key = 257ull << 32;
    int kidx = -1;
    if (ok) {
        const int lvl = predict_level(maxd, dist, s.log_scale);
        if (level_in_pyramid(lvl, s.nlevels, a.status)) {
            const float radius = a.th * s.scale[lvl];
            const uint4 q0 = s.desc[2 * i], q1 = s.desc[2 * i + 1];
            features_in_area_wave(
                F, u, v, radius, -1, -1,
                [&](int idx) {  // 1210-1211
                    const int o = F.k[idx].octave;
                    return !(o < lvl - 1 || o > lvl);
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
    if ((threadIdx.x & 63) == 0) s.vn[i] = (int)(key >> 32) <= kThHigh ? kidx : -1;  // 1224
}

// The agreement (1310-1326): match12[i1] = idx2 iff vnMatch1[i1] == idx2 >= 0 and
// vnMatch2[idx2] == i1; *nfound (zero before the launch) counts them.
__global__ __launch_bounds__(256) void sim3_agree_kernel(int n1, int n2, const int* vn1,
                                                         const int* vn2, int* match12,
                                                         int* nfound) {
    const int i1 = blockIdx.x * 256 + threadIdx.x;
    bool hit = false;
    if (i1 < n1) {
        const int i2 = vn1[i1];
        hit = i2 >= 0 && i2 < n2 && vn2[i2] == i1;
        match12[i1] = hit ? i2 : -1;
    }
    const unsigned long long b = __ballot(hit);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(nfound, __popcll(b));
}

// ---------------------------------------------------------------------------------------------
// SearchByBoW(KeyFrame* pKF1, KeyFrame* pKF2, vpMatches12) (ORBmatcher.cc:525-658): the
// (KeyFrame, Frame) search of orbfe_bow.hip with the inner side also needing a live map point
// (577-583), the strict bestDist1 < TH_LOW (601), and the result and the rotation histogram
// indexed by the KF1 feature (605, 617).  Every feature sits in exactly one node, so vbMatched2
// couples only the features of one common node: one wave per common node, in order, as there.
struct BowKkArgs {
    BowMatchArgs b;        // kf_*: pKF1 (the outer loop), f_*: pKF2; matches / bins are
                           // [P][kf_cap], indexed by the KF1 feature
    const uint8_t* f_ok;   // pKF2's features: map point present and not bad
};

// pKF1 is the outer loop and owns the result, so the search is bow_pair_search<true>
// (orbfe_bow.hip), which holds those differences as compile-time branches.
__global__ __launch_bounds__(kBowSearchBlock) void bow_search_kk_kernel(BowKkArgs k, float nnratio,
                                                                        int check_ori) {
    bow_pair_search<true>(k.b, k.f_ok, nnratio, check_ori);
}

}  // namespace orbfe

using namespace orbfe;

namespace {
int bow_kk_launch(orbfe_matcher* m, const BowKkArgs& k, int n_pairs, int gx, float nnratio,
                  int check_ori) {
    // vpMatches12 = NULL (537) per KF1 feature
    hipLaunchKernelGGL(pair_init_kernel, dim3(n_pairs), dim3(256), 0, m->stream, k.b.matches,
                       k.b.kf_cap, k.b.hist, k.b.nm, k.b.done, k.b.status);
    hipLaunchKernelGGL(bow_search_kk_kernel, dim3(gx, n_pairs), dim3(kBowSearchBlock), 0,
                       m->stream, k, nnratio, check_ori);
    ORBFE_HIP(hipGetLastError());
    return ORBFE_OK;
}
}  // namespace

extern "C" {

int orbfe_search_by_bow_keyframes(orbfe_matcher* m, float nnratio, int check_ori, int n1,
                                  const uint8_t* desc1, const float* angle1,
                                  const uint8_t* mp_ok1, int nn1, const int32_t* node_ids1,
                                  const int32_t* node_off1, const int32_t* feat1, int n2,
                                  const uint8_t* desc2, const float* angle2,
                                  const uint8_t* mp_ok2, int nn2, const int32_t* node_ids2,
                                  const int32_t* node_off2, const int32_t* feat2,
                                  int32_t* matches12, int32_t* nmatches) {
    if (n1 < 0 || n2 < 0 || nn1 < 0 || nn2 < 0 || !nmatches || (n1 && !matches12) ||
        (n1 && (!desc1 || !angle1 || !mp_ok1)) || (n2 && (!desc2 || !angle2 || !mp_ok2)) ||
        (nn1 && (!node_ids1 || !node_off1 || !feat1)) ||
        (nn2 && (!node_ids2 || !node_off2 || !feat2)))
        return ORBFE_ERR_ARG;
    if (!fv_ok(nn1, node_off1, feat1, n1) || !fv_ok(nn2, node_off2, feat2, n2))
        return ORBFE_ERR_ARG;
    const int tot1 = nn1 ? node_off1[nn1] : 0, tot2 = nn2 ? node_off2[nn2] : 0;
    return guarded(m, [&]() {
        int st;
        for (int i = 0; i < n1; ++i) matches12[i] = -1;  // vpMatches12 = NULL (537)
        *nmatches = 0;
        if (!nn1 || !nn2 || !n1 || !n2) return ORBFE_OK;
        // slot 0 of each side, the pair-indexed path with one pair; the caps bound every offset
        // and index (validated above)
        const int cap1 = std::max({n1, tot1, nn1}), cap2 = std::max({n2, tot2, nn2});
        const int nn[2] = {nn1, nn2};
        if ((st = m->up(m->fa_d, desc1, (size_t)n1 * 32))) return st;
        if ((st = m->up(m->fb_d, desc2, (size_t)n2 * 32))) return st;
        if ((st = m->up(m->m_f0, angle1, (size_t)n1 * 4))) return st;
        if ((st = m->up(m->m_f1, angle2, (size_t)n2 * 4))) return st;
        if ((st = m->up(m->m_u0, mp_ok1, n1))) return st;
        if ((st = m->up(m->m_u1, mp_ok2, n2))) return st;
        if ((st = m->up(m->m_i0, node_ids1, (size_t)nn1 * 4))) return st;
        if ((st = m->up(m->m_i1, node_off1, (size_t)(nn1 + 1) * 4))) return st;
        if ((st = m->up(m->o_i, feat1, (size_t)tot1 * 4))) return st;
        if ((st = m->up(m->fb_cs, node_ids2, (size_t)nn2 * 4))) return st;
        if ((st = m->up(m->fb_ci, node_off2, (size_t)(nn2 + 1) * 4))) return st;
        if ((st = m->up(m->fb_co, feat2, (size_t)tot2 * 4))) return st;
        if ((st = m->up(m->nq, nn, sizeof(nn)))) return st;
        if ((st = m->s1.ensure((size_t)cap1 * 4))) return st;  // bins per KF1 feature
        if ((st = m->fa_k.ensure((size_t)cap1 * 4))) return st;
        if ((st = m->scal.ensure(16))) return st;
        if ((st = m->g_hist.ensure(64 * sizeof(int)))) return st;
        BowKkArgs k{};
        BowMatchArgs& a = k.b;
        a.kf_cap = cap1;
        a.f_cap = cap2;
        a.kf_nn = m->nq.as<int>();
        a.f_nn = m->nq.as<int>() + 1;
        a.kf_node_ids = m->m_i0.as<int>();
        a.kf_node_off = m->m_i1.as<int>();
        a.kf_feat = m->o_i.as<int>();
        a.kf_ok = m->m_u0.as<uint8_t>();
        a.kf_desc = m->fa_d.as<uint4>();
        a.kf_angle = m->m_f0.as<float>();
        a.f_node_ids = m->fb_cs.as<int>();
        a.f_node_off = m->fb_ci.as<int>();
        a.f_feat = m->fb_co.as<int>();
        a.f_desc = m->fb_d.as<uint4>();
        a.f_angle = m->m_f1.as<float>();
        k.f_ok = m->m_u1.as<uint8_t>();
        a.matches = m->fa_k.as<int>();
        a.bins = m->s1.as<int>();
        a.hist = m->g_hist.as<int>();
        a.nm = m->scal.as<int>();
        a.status = m->scal.as<int>() + 1;
        a.done = m->g_hist.as<int>() + 32;
        if ((st = m->flush())) return st;
        if ((st = bow_kk_launch(m, k, 1, (nn1 + 3) / 4, nnratio, check_ori))) return st;
        int cnt[2] = {0, 0};
        if ((st = m->down(matches12, m->fa_k, (size_t)n1 * 4))) return st;
        if ((st = m->down(cnt, m->scal, sizeof(cnt)))) return st;
        if ((st = m->sync())) return st;
        *nmatches = cnt[0];
        return cnt[1];  // ORBFE_ERR_UNSUPPORTED: a KF2 node over 256 features, or a bin beyond 30
    });
}

int orbfe_search_by_bow_keyframes_batch_device(
    orbfe_matcher* m, float nnratio, int check_ori, int n_pairs, const int32_t* d_pair_kf1,
    const int32_t* d_pair_kf2, int cap, const uint8_t* d_desc, const float* d_angle,
    const uint8_t* d_mp_ok, const int32_t* d_nn, const int32_t* d_node_ids,
    const int32_t* d_node_off, const int32_t* d_feat, int32_t* d_matches12, int32_t* d_nmatches,
    int32_t* d_status) {
    if (n_pairs < 0 || n_pairs > 65535 || cap < 1 || !d_pair_kf1 || !d_pair_kf2 || !d_desc ||
        !d_angle || !d_mp_ok || !d_nn || !d_node_ids || !d_node_off || !d_feat || !d_matches12 ||
        !d_nmatches || !d_status)
        return ORBFE_ERR_ARG;
    return guarded(m, [&]() {
        int st;
        if (n_pairs == 0) {
            ORBFE_HIP(hipMemsetAsync(d_status, 0, sizeof(int32_t), m->stream));
            return ORBFE_OK;
        }
        if ((st = m->s1.ensure((size_t)n_pairs * cap * 4))) return st;
        if ((st = m->g_hist.ensure((size_t)n_pairs * 33 * sizeof(int)))) return st;
        BowKkArgs k{};
        BowMatchArgs& a = k.b;
        a.kf_cap = a.f_cap = cap;  // both sides are slots of the one keyframe set
        a.pair_kf = d_pair_kf1;
        a.pair_f = d_pair_kf2;
        a.kf_nn = a.f_nn = d_nn;
        a.kf_node_ids = a.f_node_ids = d_node_ids;
        a.kf_node_off = a.f_node_off = d_node_off;
        a.kf_feat = a.f_feat = d_feat;
        a.kf_ok = k.f_ok = d_mp_ok;
        a.kf_desc = a.f_desc = reinterpret_cast<const uint4*>(d_desc);
        a.kf_angle = a.f_angle = d_angle;
        a.matches = d_matches12;
        a.bins = m->s1.as<int>();
        a.hist = m->g_hist.as<int>();
        a.nm = d_nmatches;
        a.done = m->g_hist.as<int>() + (size_t)n_pairs * 32;
        a.status = d_status;
        // workgroups per pair as orbfe_search_by_bow_batch_device sizes them
        const int gx = std::max(1, std::min((cap + 3) / 4, (1024 + n_pairs - 1) / n_pairs));
        return bow_kk_launch(m, k, n_pairs, std::min(gx, 32), nnratio, check_ori);
    });
}

int orbfe_search_by_projection_sim3(orbfe_matcher* m, const orbfe_frame_view* kf,
                                    const float* tcw, const orbfe_camera* cam,
                                    float log_scale_factor, int n_mp, const float* mp_xyz,
                                    const float* mp_normal, const float* mp_min_dist,
                                    const float* mp_max_dist, const uint8_t* mp_desc,
                                    const uint8_t* skip, const int32_t* mp_ids, int th,
                                    int32_t* kf_matched, int32_t* nmatches) {
    // (the views are judged before the handle: a NULL matcher is guarded()'s ORBFE_ERR_ARG)
    if (!frame_ok(kf) || !tcw || !cam || !nmatches || n_mp < 0 || (kf->n && !kf_matched) ||
        (n_mp && (!mp_xyz || !mp_normal || !mp_min_dist || !mp_max_dist || !mp_desc)))
        return ORBFE_ERR_ARG;
    if (kf->nlevels > kMaxLevels) return ORBFE_ERR_UNSUPPORTED;
    return guarded(m, [&]() {
        int st;
        if ((st = m->up(m->m_f0, mp_xyz, (size_t)n_mp * 12))) return st;
        if ((st = m->up(m->m_f1, mp_normal, (size_t)n_mp * 12))) return st;
        if ((st = m->up(m->m_f2, mp_min_dist, (size_t)n_mp * 4))) return st;
        if ((st = m->up(m->m_f3, mp_max_dist, (size_t)n_mp * 4))) return st;
        if ((st = m->up(m->m_d, mp_desc, (size_t)n_mp * 32))) return st;
        if (skip && (st = m->up(m->m_u0, skip, (size_t)n_mp))) return st;
        if (mp_ids && (st = m->up(m->o_i, mp_ids, (size_t)n_mp * 4))) return st;
        // no observation counts: a keypoint holding a point before the call blocks, and so does
        // every acceptance (378, 399).  The status word: a predicted level outside the pyramid
        return sbp_search(
            m, kf, n_mp, kSbpFix, sbp_loop_cand_kernel<0>, sbp_loop_cand_kernel<1>,
            sbp_loop_cand_kernel<2>, kf_matched, nullptr, nmatches,
            [&](SbpLoopArgs& a, GreedyArgs& g, const DevFrame& F) {
                a.kf = F;
                a.n = n_mp;
                a.skip = skip ? m->m_u0.as<uint8_t>() : nullptr;
                a.xyz = m->m_f0.as<float>();
                a.normal = m->m_f1.as<float>();
                a.mind = m->m_f2.as<float>();
                a.maxd = m->m_f3.as<float>();
                a.desc = m->m_d.as<uint4>();
                put_view(a, tcw, cam, kf->min_x, kf->max_x, kf->min_y, kf->max_y);
                camera_center(tcw, a.ow);
                a.scale = m->m_f4.as<float>();
                a.nlevels = kf->nlevels;
                a.log_scale = log_scale_factor;
                a.th = (float)th;
                a.status = m->scal.as<int>() + 1;
                g.mode = kGreedyMaxD;
                g.max_dist = kThLow;
                g.ids = mp_ids ? m->o_i.as<int>() : nullptr;
            });
    });
}

int orbfe_search_by_sim3(orbfe_matcher* m, const orbfe_frame_view* kf1,
                         const orbfe_frame_view* kf2, const orbfe_camera* cam1, const float* t1w,
                         const float* t2w, const float* s12, const float* s21,
                         float log_scale_factor1, float log_scale_factor2,
                         const uint8_t* search1, const float* xyz1, const float* min_dist1,
                         const float* max_dist1, const uint8_t* desc1, const uint8_t* search2,
                         const float* xyz2, const float* min_dist2, const float* max_dist2,
                         const uint8_t* desc2, float th, int32_t* match12, int32_t* vn_match1,
                         int32_t* vn_match2, int32_t* n_found) {
    if (!frame_ok(kf1) || !frame_ok(kf2) || !cam1 || !t1w || !t2w || !s12 || !s21 ||
        !n_found ||
        (kf1->n && (!search1 || !xyz1 || !min_dist1 || !max_dist1 || !desc1 || !match12)) ||
        (kf2->n && (!search2 || !xyz2 || !min_dist2 || !max_dist2 || !desc2)))
        return ORBFE_ERR_ARG;
    if (kf1->nlevels > kMaxLevels || kf2->nlevels > kMaxLevels) return ORBFE_ERR_UNSUPPORTED;
    return guarded(m, [&]() {
        int st;
        const int n1 = kf1->n, n2 = kf2->n;
        const int32_t zero[4] = {0, 0, 0, 0};  // nFound, status
        if ((st = m->up(m->scal, zero, sizeof(zero)))) return st;
        if ((st = m->up(m->m_u0, search1, (size_t)n1))) return st;
        if ((st = m->up(m->m_f0, xyz1, (size_t)n1 * 12))) return st;
        if ((st = m->up(m->m_f1, min_dist1, (size_t)n1 * 4))) return st;
        if ((st = m->up(m->m_f2, max_dist1, (size_t)n1 * 4))) return st;
        if ((st = m->up(m->m_d, desc1, (size_t)n1 * 32))) return st;
        if ((st = m->up(m->m_u1, search2, (size_t)n2))) return st;
        if ((st = m->up(m->o_f0, xyz2, (size_t)n2 * 12))) return st;
        if ((st = m->up(m->o_f1, min_dist2, (size_t)n2 * 4))) return st;
        if ((st = m->up(m->o_f2, max_dist2, (size_t)n2 * 4))) return st;
        if ((st = m->up(m->q, desc2, (size_t)n2 * 32))) return st;
        if ((st = m->s1.ensure((size_t)std::max(n1, 1) * sizeof(int)))) return st;
        if ((st = m->s2.ensure((size_t)std::max(n2, 1) * sizeof(int)))) return st;
        if ((st = m->s3.ensure((size_t)std::max(n1, 1) * sizeof(int)))) return st;
        Sim3Args a{};
        DevFrame F1, F2;
        // the grids: a grid_kernel launch per keyframe (their image bounds may differ, and a
        // launch carries one set of bounds)
        if ((st = m->frame(kf1, false, F1))) return st;
        if ((st = m->frame(kf2, true, F2))) return st;
        Sim3Side& d12 = a.s[0];
        d12.tgt = F2;
        d12.n = n1;
        d12.search = m->m_u0.as<uint8_t>();
        d12.xyz = m->m_f0.as<float>();
        d12.mind = m->m_f1.as<float>();
        d12.maxd = m->m_f2.as<float>();
        d12.desc = m->m_d.as<uint4>();
        std::memcpy(d12.Tsw, t1w, sizeof(d12.Tsw));
        std::memcpy(d12.S, s21, sizeof(d12.S));
        d12.log_scale = log_scale_factor2;
        d12.nlevels = kf2->nlevels;
        std::memcpy(d12.scale, kf2->scale_factors, (size_t)kf2->nlevels * sizeof(float));
        d12.vn = m->s1.as<int>();
        Sim3Side& d21 = a.s[1];
        d21.tgt = F1;
        d21.n = n2;
        d21.search = m->m_u1.as<uint8_t>();
        d21.xyz = m->o_f0.as<float>();
        d21.mind = m->o_f1.as<float>();
        d21.maxd = m->o_f2.as<float>();
        d21.desc = m->q.as<uint4>();
        std::memcpy(d21.Tsw, t2w, sizeof(d21.Tsw));
        std::memcpy(d21.S, s12, sizeof(d21.S));
        d21.log_scale = log_scale_factor1;
        d21.nlevels = kf1->nlevels;
        std::memcpy(d21.scale, kf1->scale_factors, (size_t)kf1->nlevels * sizeof(float));
        d21.vn = m->s2.as<int>();
        a.fx = cam1->fx;
        a.fy = cam1->fy;
        a.cx = cam1->cx;
        a.cy = cam1->cy;
        a.th = th;
        a.status = m->scal.as<int>() + 1;
        if ((st = m->flush())) return st;
        const int nmax = std::max(n1, n2);
        if (nmax > 0)
            hipLaunchKernelGGL(sim3_search_kernel, dim3((nmax + 3) / 4, 2), dim3(256), 0, m->stream, a);
        if (n1 > 0)
            hipLaunchKernelGGL(sim3_agree_kernel, dim3((n1 + 255) / 256), dim3(256), 0, m->stream,
                               n1, n2, m->s1.as<int>(), m->s2.as<int>(), m->s3.as<int>(),
                               m->scal.as<int>());
        ORBFE_HIP(hipGetLastError());
        if ((st = m->down(match12, m->s3, (size_t)n1 * 4))) return st;
        if (vn_match1 && (st = m->down(vn_match1, m->s1, (size_t)n1 * 4))) return st;
        if (vn_match2 && (st = m->down(vn_match2, m->s2, (size_t)n2 * 4))) return st;
        int res[2] = {0, 0};  // {nFound, status}
        if ((st = m->down(res, m->scal, sizeof(res)))) return st;
        if ((st = m->sync())) return st;
        *n_found = res[0];
        return res[1];
    });
}

}  // extern "C"
