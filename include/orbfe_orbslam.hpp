// orbfe_orbslam.hpp — header-only C++ mirror of ORB-SLAM2's ORBextractor / ORBmatcher
// interface over the C ABI (include/orbfe.h), for host code that is compiled C++ like the
// reference.  Names, argument meaning and ordering follow include/ORBextractor.h:50-119 and
// include/ORBmatcher.h:38-110 of skaegy/ORBSLAM_MapSave; OpenCV types are replaced by plain
// buffers (INTEGRATION.md shows the cv::Mat glue).  Errors surface as orbfe::Error exceptions
// on the C++ side only; nothing throws across the C ABI.
#pragma once

#include <algorithm>
#include <array>
#include <cmath>
#include <list>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include "orbfe.h"

namespace orbfe {

struct Error : std::runtime_error {
    int status;
    Error(const char* fn, int st)
        : std::runtime_error(std::string(fn) + " failed with status " + std::to_string(st)),
          status(st) {}
};

inline void check(const char* fn, int st) {
    if (st != ORBFE_OK) throw Error(fn, st);
}

// ORB_SLAM2::ORBextractor (ORBextractor.h:50-119) on a gfx950 GPU.
class ORBextractor {
public:
    enum { HARRIS_SCORE = 0, FAST_SCORE = 1 };

    ORBextractor(int nfeatures, float scaleFactor, int nlevels, int iniThFAST, int minThFAST,
                 int device = 0, int max_width = 0, int max_height = 0)
        : nlevels_(nlevels) {
        orbfe_params p{nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST};
        int st = ORBFE_OK;
        h_ = orbfe_create(&p, device, max_width, max_height, 1, &st);
        if (!h_) throw Error("orbfe_create", st);
    }
    ~ORBextractor() { orbfe_destroy(h_); }
    ORBextractor(const ORBextractor&) = delete;
    ORBextractor& operator=(const ORBextractor&) = delete;

    // operator()(image, mask, keypoints, descriptors) (ORBextractor.cc:1042-1108):
    // image = rows x cols u8 with row step `step`; mask NULL or same size.  An empty image
    // leaves the outputs untouched; zero keypoints clears both.
    void operator()(const uint8_t* image, int cols, int rows, size_t step, const uint8_t* mask,
                    size_t mask_step, std::vector<orbfe_keypoint>& keypoints,
                    std::vector<uint8_t>& descriptors) {
        if (!image || cols <= 0 || rows <= 0) return;
        const int cap = orbfe_keypoint_capacity_for(h_, cols, rows);
        if (cap < 0) throw Error("orbfe_keypoint_capacity_for", cap);
        keypoints.resize(cap);
        descriptors.resize((size_t)cap * 32);
        int n = 0;
        check("orbfe_extract", orbfe_extract(h_, image, cols, rows, step, mask, mask_step,
                                             keypoints.data(), cap, descriptors.data(), &n));
        keypoints.resize(n);
        descriptors.resize((size_t)n * 32);
    }

    // Zero-copy form (orbfe_input_buffer / orbfe_extract_staged): the caller writes the gray
    // frame into InputBuffer (GrabImageMonocular's cvtColor target, Tracking.cc:409-422), then
    // ExtractStaged runs operator() on it in place (Frame::ExtractORB, Frame.cc:358-364).
    uint8_t* InputBuffer(int cols, int rows, size_t* step) {
        uint8_t* buf = nullptr;
        check("orbfe_input_buffer", orbfe_input_buffer(h_, cols, rows, &buf, step));
        return buf;
    }
    void ExtractStaged(int cols, int rows, std::vector<orbfe_keypoint>& keypoints,
                       std::vector<uint8_t>& descriptors) {
        int n = 0;
        check("orbfe_extract_staged", orbfe_extract_staged(h_, cols, rows, nullptr, 0, nullptr, &n));
        const orbfe_keypoint* k = nullptr;
        const uint8_t* d = nullptr;
        check("orbfe_staged_outputs", orbfe_staged_outputs(h_, &k, &d, &n));
        keypoints.assign(k, k + n);
        descriptors.assign(d, d + (size_t)n * 32);
    }

    // Frame::ComputeStereoFromRGBD (Frame.cc:759-780) on the raw depth image as the grabber
    // delivers it (depth_type ORBFE_DEPTH_U16 / ORBFE_DEPTH_F32) with the conversion
    // imDepth.convertTo(imDepth, CV_32F, mDepthMapFactor) (Tracking.cc:367-368) fused: fills
    // mvuRight / mvDepth.  mvKeysUn empty: mvKeysUn = mvKeys (Frame::UndistortKeyPoints with
    // k1 == 0).  A keypoint outside the depth image gets -1 / -1 and the call throws
    // ORBFE_ERR_UNSUPPORTED after filling the others.
    void ComputeStereoFromRGBD(const void* imDepth, int depth_type, int cols, int rows, size_t step,
                               float depthMapFactor, const std::vector<orbfe_keypoint>& mvKeys,
                               const std::vector<orbfe_keypoint>& mvKeysUn, float mbf,
                               std::vector<float>& mvuRight, std::vector<float>& mvDepth) {
        if (!mvKeysUn.empty() && mvKeysUn.size() != mvKeys.size())
            throw Error("ORBextractor::ComputeStereoFromRGBD", ORBFE_ERR_ARG);
        mvuRight.assign(mvKeys.size(), -1.f);  // 761-762
        mvDepth.assign(mvKeys.size(), -1.f);
        check("orbfe_compute_stereo_from_rgbd",
              orbfe_compute_stereo_from_rgbd(h_, imDepth, depth_type, cols, rows, step, depthMapFactor,
                                             mvKeys.data(), mvKeysUn.empty() ? nullptr : mvKeysUn.data(),
                                             (int)mvKeys.size(), mbf, mvuRight.data(), mvDepth.data()));
    }
    // The depth twin of InputBuffer: the grabber writes the raw depth image into it and
    // ComputeStereoFromRGBD, given this pointer, gathers from it in place.
    void* DepthBuffer(int cols, int rows, int depth_type, size_t* step) {
        void* buf = nullptr;
        check("orbfe_depth_buffer", orbfe_depth_buffer(h_, cols, rows, depth_type, &buf, step));
        return buf;
    }

    int GetLevels() { return orbfe_get_levels(h_); }
    float GetScaleFactor() { return orbfe_get_scale_factor(h_); }
    std::vector<float> GetScaleFactors() { return table(0); }
    std::vector<float> GetInverseScaleFactors() { return table(1); }
    std::vector<float> GetScaleSigmaSquares() { return table(2); }
    std::vector<float> GetInverseScaleSigmaSquares() { return table(3); }

    // mvImagePyramid[level] of the last call (ORBextractor.h:90): rows x cols, dense.
    std::vector<uint8_t> ImagePyramidLevel(int level, int* cols, int* rows) {
        int w = 0, h = 0;
        check("orbfe_get_level", orbfe_get_level(h_, 0, level, nullptr, &w, &h));
        std::vector<uint8_t> out((size_t)w * h);
        check("orbfe_get_level", orbfe_get_level(h_, 0, level, out.data(), &w, &h));
        if (cols) *cols = w;
        if (rows) *rows = h;
        return out;
    }

    orbfe_extractor* handle() { return h_; }

private:
    std::vector<float> table(int which) {
        std::vector<float> t[4];
        for (auto& v : t) v.resize(nlevels_);
        check("orbfe_get_scale_tables",
              orbfe_get_scale_tables(h_, t[0].data(), t[1].data(), t[2].data(), t[3].data()));
        return t[which];
    }
    orbfe_extractor* h_ = nullptr;
    int nlevels_;
};

// Flat stand-in for the Frame members the matchers read (Frame.h): owns nothing.
// A DBoW2 FeatureVector (node id -> feature indices, ids ascending) as flat arrays: node i's
// features are feat[node_off[i] .. node_off[i + 1]).
struct FeatureVectorView {
    const int32_t* node_ids;
    const int32_t* node_off;  // nn + 1
    const int32_t* feat;
    int nn;
};

struct FrameData {
    std::vector<orbfe_keypoint> keys_un;   // mvKeysUn
    std::vector<uint8_t> descriptors;      // mDescriptors, N x 32
    std::vector<float> u_right;            // mvuRight (empty: monocular)
    float min_x = 0, max_x = 0, min_y = 0, max_y = 0;  // mnMinX ... (Frame.cc:554-582)
    std::vector<float> scale_factors;      // mvScaleFactors
    std::vector<int> map_points;           // mvpMapPoints as MapPoint ids, -1 = NULL
    std::vector<int> map_point_obs;        // Observations() of those MapPoints

    orbfe_frame_view view() const {
        orbfe_frame_view v;
        v.n = (int)keys_un.size();
        v.keys_un = keys_un.data();
        v.desc = descriptors.data();
        v.u_right = u_right.empty() ? nullptr : u_right.data();
        v.min_x = min_x;
        v.max_x = max_x;
        v.min_y = min_y;
        v.max_y = max_y;
        v.grid_w_inv = 64.f / (max_x - min_x);  // FRAME_GRID_COLS / width (Frame.cc:212)
        v.grid_h_inv = 48.f / (max_y - min_y);
        v.scale_factors = scale_factors.data();
        v.nlevels = (int)scale_factors.size();
        return v;
    }
};

// The MapPoints handed to ORBmatcher::Fuse as flat arrays (owns nothing): GetWorldPos() and
// GetNormal() (n x 3), mfMinDistance / mfMaxDistance, GetDescriptor() (n x 32).  skip: NULL or
// n bytes, the skip test as it stands before the call (saves the search of those points; the
// walk asks the live test again either way).
struct FusePoints {
    int n = 0;
    const float* xyz = nullptr;
    const float* normal = nullptr;
    const float* min_dist = nullptr;
    const float* max_dist = nullptr;
    const uint8_t* desc = nullptr;
    const uint8_t* skip = nullptr;
};

// The KeyFrame members ORBmatcher::SearchForTriangulation reads (owns nothing): the frame data,
// mFeatVec, GetMapPoint(i) != NULL per feature, GetRotation() (3 x 3 row-major), GetTranslation(),
// GetCameraCenter(), the intrinsics and mvLevelSigma2 (frame->scale_factors.size() floats).
struct KeyFrameData {
    const FrameData* frame = nullptr;
    FeatureVectorView feat_vec{nullptr, nullptr, nullptr, 0};
    const uint8_t* has_map_point = nullptr;
    const float* Rcw = nullptr;
    const float* tcw = nullptr;
    const float* Ow = nullptr;
    float fx = 0, fy = 0, cx = 0, cy = 0;
    const float* level_sigma2 = nullptr;
};

// The map points a keyframe's features hold (pKF->GetMapPointMatches()) as flat arrays, one entry
// per feature (owns nothing): ids (-1 = NULL), isBad(), GetWorldPos() (n x 3), mfMinDistance /
// mfMaxDistance and GetDescriptor() (n x 32).  Entries of a NULL slot are not read.
struct KeyFramePoints {
    const int* ids = nullptr;
    const uint8_t* bad = nullptr;
    const float* xyz = nullptr;
    const float* min_dist = nullptr;
    const float* max_dist = nullptr;
    const uint8_t* desc = nullptr;
};

// Rows 0-2 of the 4x4 Sim3 matrix Scw = [s R | t] (row-major 3x4), LoopClosing's corrected pose.
struct Sim3 {
    float m[12];
};

// What the close-point loops of Tracking visit (ORBmatcher::ClosePoints): visit j is feature
// order[j]; where create[j], a new MapPoint goes to xyz[3 j ..] with mfMaxDistance / mfMinDistance
// max_dist[j] / min_dist[j].  n_total / n_map: nTotal / nMap of Tracking::NeedNewKeyFrame.
struct ClosePointsResult {
    std::vector<int> order;
    std::vector<uint8_t> create;
    std::vector<float> xyz, max_dist, min_dist;
    int n_total = 0, n_map = 0;
    bool octave_out_of_pyramid = false;  // a created visit indexed mvScaleFactors out of range
};

// ORB_SLAM2::ORBmatcher hot subset (ORBmatcher.h:38-110) on a gfx950 GPU.
class ORBmatcher {
public:
    static const int TH_HIGH = 100, TH_LOW = 50, HISTO_LENGTH = 30;  // ORBmatcher.cc:37-39

    explicit ORBmatcher(float nnratio = 0.6f, bool checkOri = true, int device = 0)
        : mfNNratio(nnratio), mbCheckOrientation(checkOri) {
        int st = ORBFE_OK;
        m_ = orbfe_matcher_create(device, &st);
        if (!m_) throw Error("orbfe_matcher_create", st);
    }
    ~ORBmatcher() { orbfe_matcher_destroy(m_); }
    ORBmatcher(const ORBmatcher&) = delete;
    ORBmatcher& operator=(const ORBmatcher&) = delete;

    // DescriptorDistance (ORBmatcher.cc:1650-1666), batched: dist[i] = H(a_i, b_i).
    std::vector<int> DescriptorDistance(const uint8_t* a, const uint8_t* b, int n) {
        std::vector<int> d(n);
        check("orbfe_hamming", orbfe_hamming(m_, a, b, n, d.data()));
        return d;
    }

    // SearchForInitialization (ORBmatcher.cc:408-523); vbPrevMatched holds (x, y) pairs.
    int SearchForInitialization(const FrameData& F1, const FrameData& F2,
                                std::vector<float>& vbPrevMatched, std::vector<int>& vnMatches12,
                                int windowSize = 10) {
        vnMatches12.assign(F1.keys_un.size(), -1);
        const orbfe_frame_view v1 = F1.view(), v2 = F2.view();
        int n = 0;
        check("orbfe_search_for_initialization",
              orbfe_search_for_initialization(m_, mfNNratio, mbCheckOrientation, &v1, &v2,
                                              vbPrevMatched.data(), windowSize,
                                              vnMatches12.data(), &n));
        return n;
    }

    // SearchByProjection(Frame& F, const vector<MapPoint*>&, th) (ORBmatcher.cc:45-129).
    int SearchByProjection(FrameData& F, const orbfe_mappoint_view& mps, const int* mp_ids,
                           float th = 3) {
        prepare(F);
        const orbfe_frame_view v = F.view();
        int n = 0;
        check("orbfe_search_by_projection_local",
              orbfe_search_by_projection_local(m_, mfNNratio, &v, F.map_points.data(),
                                               F.map_point_obs.data(), &mps, mp_ids, th, &n));
        return n;
    }

    // SearchByProjection(Frame& Cur, const Frame& Last, th, bMono) (ORBmatcher.cc:1331-1473).
    // last_*: per last-frame keypoint, the MapPoint it holds (valid flag, world position,
    // descriptor, Observations(), id) and mvbOutlier; poses are row-major 3x4 world->camera.
    int SearchByProjection(FrameData& Cur, const float* Tcw, const orbfe_camera& cam,
                           const FrameData& Last, const std::vector<uint8_t>& last_valid,
                           const std::vector<uint8_t>& last_outlier,
                           const std::vector<float>& last_xyz,
                           const std::vector<uint8_t>& last_desc,
                           const std::vector<int>& last_nobs, const std::vector<int>& last_ids,
                           const float* Tlw, float th, bool bMono) {
        prepare(Cur);
        const orbfe_frame_view v = Cur.view();
        int n = 0;
        check("orbfe_search_by_projection_last",
              orbfe_search_by_projection_last(
                  m_, mbCheckOrientation, &v, Tcw, &cam, Cur.map_points.data(),
                  Cur.map_point_obs.data(), (int)Last.keys_un.size(), Last.keys_un.data(),
                  last_valid.data(), last_outlier.data(), last_xyz.data(), last_desc.data(),
                  last_nobs.data(), last_ids.empty() ? nullptr : last_ids.data(), Tlw, th,
                  bMono, &n));
        return n;
    }

    // SearchByBoW(KeyFrame* pKF, Frame& F, vpMapPointMatches) (ORBmatcher.cc:159-291).
    // kf_mp_ok[i]: the keyframe's feature i holds a MapPoint that is not bad (202-207); the two
    // FeatureVectors as their (node id, features) lists; vpMapPointMatches[f] = the keyframe
    // feature matched to frame feature f, or -1.
    int SearchByBoW(const FrameData& KF, const std::vector<uint8_t>& kf_mp_ok,
                    const FeatureVectorView& kf_fv, const FrameData& F,
                    const FeatureVectorView& f_fv, std::vector<int>& vpMapPointMatches) {
        kf_angle_.resize(KF.keys_un.size());
        for (size_t i = 0; i < KF.keys_un.size(); ++i) kf_angle_[i] = KF.keys_un[i].angle;
        f_angle_.resize(F.keys_un.size());
        for (size_t i = 0; i < F.keys_un.size(); ++i) f_angle_[i] = F.keys_un[i].angle;
        vpMapPointMatches.resize(F.keys_un.size());
        int n = 0;
        check("orbfe_search_by_bow",
              orbfe_search_by_bow(m_, mfNNratio, mbCheckOrientation, (int)KF.keys_un.size(),
                                  KF.descriptors.data(), kf_angle_.data(), kf_mp_ok.data(),
                                  kf_fv.nn, kf_fv.node_ids, kf_fv.node_off, kf_fv.feat,
                                  (int)F.keys_un.size(), F.descriptors.data(), f_angle_.data(),
                                  f_fv.nn, f_fv.node_ids, f_fv.node_off, f_fv.feat,
                                  vpMapPointMatches.data(), &n));
        return n;
    }

    // Fuse(KeyFrame* pKF, const vector<MapPoint*>& vpMapPoints, th) (ORBmatcher.cc:828-978), as
    // LocalMapping::SearchInNeighbors calls it.  The device searches every point at once
    // (orbfe_fuse_search); the tail of the loop (955-974) is the caller's, through callables, in
    // the order of the list:
    //   skipped(i)          !pMP || pMP->isBad() || pMP->IsInKeyFrame(pKF), asked when the walk
    //                       reaches i — a Replace earlier in the walk can change it
    //   slot_occupied(idx)  pKF->GetMapPoint(idx) != NULL
    //   on_occupied(i, idx) lines 958-966: the two Replace directions, unless pMPinKF is bad
    //   on_empty(i, idx)    lines 970-971: AddObservation + AddMapPoint
    // Returns nFused.  A predicted level outside the pyramid throws Error(ORBFE_ERR_UNSUPPORTED)
    // before any callable runs.
    template <class Skipped, class Occupied, class OnOccupied, class OnEmpty>
    int Fuse(const FrameData& KF, const float* Tcw, const orbfe_camera& cam,
             float logScaleFactor, const std::vector<float>& invLevelSigma2,
             const FusePoints& pts, float th, Skipped skipped, Occupied slot_occupied,
             OnOccupied on_occupied, OnEmpty on_empty) {
        return fuse(KF, Tcw, cam, logScaleFactor, invLevelSigma2, pts, th, ORBFE_FUSE_SE3,
                    skipped, slot_occupied, on_occupied, on_empty);
    }

    // Fuse(KeyFrame* pKF, cv::Mat Scw, const vector<MapPoint*>& vpPoints, th, vpReplacePoint)
    // (ORBmatcher.cc:980-1103), as LoopClosing::SearchAndFuse calls it.  Scw is decomposed here
    // as lines 989-992 do: scw = (float)sqrt of the double dot product of row 0, Rcw = sRcw / scw
    // and tcw = t / scw as products with the float (float)(1.0 / scw) (cv::Mat / double scales
    // by the reciprocal).  skipped(i) is pMP->isBad() ||
    // spAlreadyFound.count(pMP); on_occupied(i, idx) is lines 1090-1091 (vpReplacePoint[i] =
    // pMPinKF unless it is bad), on_empty(i, idx) lines 1095-1096.  inv_level_sigma2 is not read.
    template <class Skipped, class Occupied, class OnOccupied, class OnEmpty>
    int Fuse(const FrameData& KF, const Sim3& Scw, const orbfe_camera& cam, float logScaleFactor,
             const FusePoints& pts, float th, Skipped skipped, Occupied slot_occupied,
             OnOccupied on_occupied, OnEmpty on_empty) {
        float T[12];
        normalise(Scw, T);
        const std::vector<float> unused(KF.scale_factors.size(), 0.f);
        return fuse(KF, T, cam, logScaleFactor, unused, pts, th, ORBFE_FUSE_SIM3, skipped,
                    slot_occupied, on_occupied, on_empty);
    }

    // SearchForTriangulation(KeyFrame* pKF1, KeyFrame* pKF2, cv::Mat F12, vMatchedPairs,
    // bOnlyStereo) (ORBmatcher.cc:660-826), as LocalMapping::CreateNewMapPoints calls it with
    // F12 = ComputeF12(pKF1, pKF2), 3 x 3 row-major.  The epipole is evaluated here as lines
    // 667-673 write it: C2 = R2w * Cw + t2w is one cv::gemm (products and the added t2w
    // accumulated in double, rounded to float once per element), invz, ex and ey are float
    // expressions.  vMatchedPairs receives vMatches12 compacted in ascending keyframe-1 index;
    // returns nmatches.  blockMatched2 = false is the reference as written (vbMatched2 is read
    // but never set, so a keyframe-2 feature can appear in several pairs); true blocks a
    // matched keyframe-2 feature for the rest of its node, the evident intent.
    int SearchForTriangulation(const KeyFrameData& KF1, const KeyFrameData& KF2, const float* F12,
                               std::vector<std::pair<size_t, size_t>>& vMatchedPairs,
                               bool bOnlyStereo, bool blockMatched2 = false) {
        if (!KF1.frame || !KF2.frame || !KF1.Ow || !KF2.Rcw || !KF2.tcw)
            throw Error("ORBmatcher::SearchForTriangulation", ORBFE_ERR_ARG);
        float C2[3];
        for (int r = 0; r < 3; ++r)
            C2[r] = (float)((double)KF2.Rcw[3 * r] * KF1.Ow[0] + (double)KF2.Rcw[3 * r + 1] * KF1.Ow[1] +
                            (double)KF2.Rcw[3 * r + 2] * KF1.Ow[2] + (double)KF2.tcw[r]);
        const float invz = 1.0f / C2[2];
        const float epipole[2] = {KF2.fx * C2[0] * invz + KF2.cx, KF2.fy * C2[1] * invz + KF2.cy};
        const orbfe_frame_view v1 = KF1.frame->view(), v2 = KF2.frame->view();
        tri_m12_.assign(v1.n, -1);
        int n = 0;
        check("orbfe_search_for_triangulation",
              orbfe_search_for_triangulation(
                  m_, mbCheckOrientation, blockMatched2, bOnlyStereo, &v1, KF1.has_map_point,
                  KF1.feat_vec.nn, KF1.feat_vec.node_ids, KF1.feat_vec.node_off, KF1.feat_vec.feat,
                  &v2, KF2.has_map_point, KF2.feat_vec.nn, KF2.feat_vec.node_ids,
                  KF2.feat_vec.node_off, KF2.feat_vec.feat, F12, epipole, KF2.level_sigma2,
                  tri_m12_.data(), &n));
        vMatchedPairs.clear();
        vMatchedPairs.reserve(n);
        for (size_t i = 0; i < tri_m12_.size(); ++i)
            if (tri_m12_[i] >= 0) vMatchedPairs.push_back(std::make_pair(i, (size_t)tri_m12_[i]));
        return n;
    }

    // SearchByBoW(KeyFrame* pKF1, KeyFrame* pKF2, vector<MapPoint*>& vpMatches12)
    // (ORBmatcher.cc:525-658), as LoopClosing::ComputeSim3 calls it per loop candidate.  Only
    // ids and bad of P1 / P2 are read (a feature takes part when it holds a point that is not
    // bad, 561-565 and 577-583); fv1 / fv2 are the keyframes' mFeatVec.  vpMatches12 is
    // overwritten: KF1.keys_un.size() entries, P2.ids[idx2] for a match, -1 = NULL.  Returns
    // nmatches.
    int SearchByBoW(const FrameData& KF1, const KeyFramePoints& P1, const FeatureVectorView& fv1,
                    const FrameData& KF2, const KeyFramePoints& P2, const FeatureVectorView& fv2,
                    std::vector<int>& vpMatches12) {
        const size_t N1 = KF1.keys_un.size(), N2 = KF2.keys_un.size();
        kf_angle_.resize(N1);
        sim3_search1_.resize(N1);
        for (size_t i = 0; i < N1; ++i) {
            kf_angle_[i] = KF1.keys_un[i].angle;
            sim3_search1_[i] = P1.ids[i] >= 0 && !P1.bad[i];
        }
        f_angle_.resize(N2);
        sim3_search2_.resize(N2);
        for (size_t i = 0; i < N2; ++i) {
            f_angle_[i] = KF2.keys_un[i].angle;
            sim3_search2_[i] = P2.ids[i] >= 0 && !P2.bad[i];
        }
        sim3_m12_.assign(N1, -1);
        int n = 0;
        check("orbfe_search_by_bow_keyframes",
              orbfe_search_by_bow_keyframes(
                  m_, mfNNratio, mbCheckOrientation, (int)N1, KF1.descriptors.data(),
                  kf_angle_.data(), sim3_search1_.data(), fv1.nn, fv1.node_ids, fv1.node_off,
                  fv1.feat, (int)N2, KF2.descriptors.data(), f_angle_.data(),
                  sim3_search2_.data(), fv2.nn, fv2.node_ids, fv2.node_off, fv2.feat,
                  sim3_m12_.data(), &n));
        vpMatches12.assign(N1, -1);
        for (size_t i = 0; i < N1; ++i)
            if (sim3_m12_[i] >= 0) vpMatches12[i] = P2.ids[sim3_m12_[i]];
        return n;
    }

    // SearchByProjection(KeyFrame* pKF, cv::Mat Scw, const vector<MapPoint*>& vpPoints,
    // vector<MapPoint*>& vpMatched, int th) (ORBmatcher.cc:293-406), as LoopClosing::ComputeSim3
    // calls it (th = 10).  Scw is decomposed as for Fuse (302-305).  pts.skip is isBad() per
    // point (NULL: none is bad); spAlreadyFound (309-310) is built here, once, from vpMatched as
    // it stands before the call and mp_ids (NULL: a point's id is its index in the list), so a
    // point listed twice can match twice, as in the reference.  vpMatched: KF's keypoint slots as
    // ids, -1 = NULL; a match writes the point's id.  Returns nmatches.  A predicted level
    // outside the pyramid throws Error(ORBFE_ERR_UNSUPPORTED) with vpMatched updated for every
    // other point.
    int SearchByProjection(const FrameData& KF, const Sim3& Scw, const orbfe_camera& cam,
                           float logScaleFactor, const FusePoints& pts, const int* mp_ids,
                           std::vector<int>& vpMatched, int th) {
        float T[12];
        normalise(Scw, T);
        vpMatched.resize(KF.keys_un.size(), -1);
        std::vector<int> found(vpMatched);
        std::sort(found.begin(), found.end());
        loop_skip_.assign(pts.n, 0);
        for (int i = 0; i < pts.n; ++i) {
            const int id = mp_ids ? mp_ids[i] : i;
            loop_skip_[i] = (pts.skip && pts.skip[i]) ||
                            (id >= 0 && std::binary_search(found.begin(), found.end(), id));
        }
        const orbfe_frame_view v = KF.view();
        int n = 0;
        check("orbfe_search_by_projection_sim3",
              orbfe_search_by_projection_sim3(m_, &v, T, &cam, logScaleFactor, pts.n, pts.xyz,
                                              pts.normal, pts.min_dist, pts.max_dist, pts.desc,
                                              loop_skip_.data(), mp_ids, th, vpMatched.data(), &n));
        return n;
    }

    // SearchBySim3(KeyFrame* pKF1, KeyFrame* pKF2, vector<MapPoint*>& vpMatches12, s12, R12, t12,
    // th) (ORBmatcher.cc:1105-1329), as the RANSAC loop of LoopClosing::ComputeSim3 calls it
    // (th = 7.5).  T1w / T2w: the keyframes' row-major 3x4 [R|t]; R12 3 x 3 row-major, t12 3.
    // Lines 1122-1124 are evaluated here: sR12 = every entry times the float s12, sR21 = every
    // entry of R12^T times (float)(1.0 / (double)s12), t21 = -((a0 t0 + a1 t1) + a2 t2) per row
    // (DESIGN.md H16).  vpMatches12: KF1.keys_un.size() ids, -1 = NULL, as it stands before the
    // call; index_in_kf2(id) is pMP->GetIndexInKeyFrame(pKF2) for such an id.  The agreeing
    // pairs (1310-1326) are written as vpMatches12[i1] = P2.ids[idx2]; returns nFound.
    template <class IndexInKF2>
    int SearchBySim3(const FrameData& KF1, const KeyFramePoints& P1, const float* T1w,
                     float logScaleFactor1, const FrameData& KF2, const KeyFramePoints& P2,
                     const float* T2w, float logScaleFactor2, const orbfe_camera& cam1,
                     std::vector<int>& vpMatches12, float s12, const float* R12, const float* t12,
                     float th, IndexInKF2 index_in_kf2) {
        const int N1 = (int)KF1.keys_un.size(), N2 = (int)KF2.keys_un.size();
        vpMatches12.resize(N1, -1);
        float S12[12], S21[12];
        const float inv = (float)(1.0 / (double)s12);
        for (int r = 0; r < 3; ++r) {
            for (int c = 0; c < 3; ++c) {
                S12[4 * r + c] = s12 * R12[3 * r + c];
                S21[4 * r + c] = R12[3 * c + r] * inv;
            }
            S12[4 * r + 3] = t12[r];
        }
        for (int r = 0; r < 3; ++r)
            S21[4 * r + 3] = -((S21[4 * r] * t12[0] + S21[4 * r + 1] * t12[1]) + S21[4 * r + 2] * t12[2]);
        sim3_search1_.assign(N1, 0);
        sim3_search2_.assign(N2, 0);
        for (int i = 0; i < N2; ++i) sim3_search2_[i] = P2.ids[i] >= 0 && !P2.bad[i];
        for (int i = 0; i < N1; ++i) {
            sim3_search1_[i] = P1.ids[i] >= 0 && !P1.bad[i] && vpMatches12[i] < 0;
            if (vpMatches12[i] >= 0) {  // 1135-1145
                const int idx2 = index_in_kf2(vpMatches12[i]);
                if (idx2 >= 0 && idx2 < N2) sim3_search2_[idx2] = 0;
            }
        }
        sim3_m12_.assign(N1, -1);
        const orbfe_frame_view v1 = KF1.view(), v2 = KF2.view();
        int n = 0;
        check("orbfe_search_by_sim3",
              orbfe_search_by_sim3(m_, &v1, &v2, &cam1, T1w, T2w, S12, S21, logScaleFactor1,
                                   logScaleFactor2, sim3_search1_.data(), P1.xyz, P1.min_dist,
                                   P1.max_dist, P1.desc, sim3_search2_.data(), P2.xyz, P2.min_dist,
                                   P2.max_dist, P2.desc, th, sim3_m12_.data(), nullptr, nullptr,
                                   &n));
        for (int i = 0; i < N1; ++i)
            if (sim3_m12_[i] >= 0) vpMatches12[i] = P2.ids[sim3_m12_[i]];
        return n;
    }

    // The close-point loop of Tracking::UpdateLastFrame (Tracking.cc:1059-1111) and
    // CreateNewKeyFrame (1333-1392) with mode ORBFE_CLOSE_SORTED, StereoInitialization's
    // (764-779) with ORBFE_CLOSE_ALL, over F.keys_un / mvDepth, creating with
    // Frame::UnprojectStereo (Frame.cc:782-796).  F.map_points / F.map_point_obs give
    // "mvpMapPoints[i] && Observations() >= 1" (both empty: no MapPoints).  Rwc (3 x 3 row-major)
    // and Ow are the products of Frame::UpdatePoseMatrices.  The caller walks the result and does
    // the `new MapPoint` bookkeeping.
    ClosePointsResult ClosePoints(int mode, const FrameData& F, const std::vector<float>& mvDepth,
                                  const orbfe_camera& cam, const float* Rwc, const float* Ow,
                                  float thDepth, int minPoints = 100) {
        const size_t N = F.keys_un.size();
        if (mvDepth.size() != N || !Rwc || !Ow || (!F.map_points.empty() && F.map_points.size() != N) ||
            (!F.map_points.empty() && F.map_point_obs.size() != N))
            throw Error("ORBmatcher::ClosePoints", ORBFE_ERR_ARG);
        std::vector<uint8_t> has_point(N, 0);
        for (size_t i = 0; i < N && !F.map_points.empty(); ++i)
            has_point[i] = F.map_points[i] >= 0 && F.map_point_obs[i] >= 1;
        float pose[12];
        std::copy(Rwc, Rwc + 9, pose);
        std::copy(Ow, Ow + 3, pose + 9);
        ClosePointsResult r;
        r.order.resize(N);
        r.create.resize(N);
        r.xyz.resize(3 * N);
        r.max_dist.resize(N);
        r.min_dist.resize(N);
        int visited = 0;
        const int st = orbfe_close_points(
            m_, mode, F.keys_un.data(), mvDepth.data(), has_point.data(), (int)N, &cam, pose, thDepth,
            minPoints, F.scale_factors.data(), (int)F.scale_factors.size(), r.order.data(), &visited,
            r.create.data(), r.xyz.data(), r.max_dist.data(), r.min_dist.data(), &r.n_total, &r.n_map);
        if (st != ORBFE_OK && st != ORBFE_ERR_UNSUPPORTED) throw Error("orbfe_close_points", st);
        r.octave_out_of_pyramid = st == ORBFE_ERR_UNSUPPORTED;
        r.order.resize(visited);
        r.create.resize(visited);
        r.xyz.resize(3 * (size_t)visited);
        r.max_dist.resize(visited);
        r.min_dist.resize(visited);
        return r;
    }

    orbfe_matcher* handle() { return m_; }

private:
    template <class Skipped, class Occupied, class OnOccupied, class OnEmpty>
    int fuse(const FrameData& KF, const float* T, const orbfe_camera& cam, float logScaleFactor,
             const std::vector<float>& invLevelSigma2, const FusePoints& pts, float th, int mode,
             Skipped& skipped, Occupied& slot_occupied, OnOccupied& on_occupied,
             OnEmpty& on_empty) {
        if (invLevelSigma2.size() < KF.scale_factors.size()) throw Error("ORBmatcher::Fuse", ORBFE_ERR_ARG);
        const orbfe_frame_view v = KF.view();
        fuse_idx_.assign(pts.n, -1);
        int found = 0;
        check("orbfe_fuse_search",
              orbfe_fuse_search(m_, &v, T, &cam, logScaleFactor, invLevelSigma2.data(), pts.n,
                                pts.xyz, pts.normal, pts.min_dist, pts.max_dist, pts.desc,
                                pts.skip, th, mode, fuse_idx_.data(), nullptr, &found));
        int nFused = 0;
        for (int i = 0; i < pts.n; ++i) {
            if (skipped(i)) continue;
            const int idx = fuse_idx_[i];
            if (idx < 0) continue;
            if (slot_occupied(idx))
                on_occupied(i, idx);
            else
                on_empty(i, idx);
            ++nFused;
        }
        return nFused;
    }
    // Scw -> the normalised [Rcw|tcw] of ORBmatcher.cc:302-305 / 989-992.
    static void normalise(const Sim3& Scw, float T[12]) {
        const float* s = Scw.m;
        const float scw = (float)std::sqrt((double)s[0] * s[0] + (double)s[1] * s[1] + (double)s[2] * s[2]);
        const float inv = (float)(1.0 / (double)scw);
        for (int i = 0; i < 12; ++i) T[i] = s[i] * inv;
    }
    static void prepare(FrameData& F) {
        F.map_points.resize(F.keys_un.size(), -1);
        F.map_point_obs.resize(F.keys_un.size(), 0);
    }
    orbfe_matcher* m_ = nullptr;
    float mfNNratio;
    bool mbCheckOrientation;
    std::vector<float> kf_angle_, f_angle_;  // SearchByBoW: the keypoints' angles as arrays
    std::vector<int> fuse_idx_;              // Fuse: best_idx of the device search
    std::vector<int> tri_m12_;               // SearchForTriangulation: vMatches12
    std::vector<uint8_t> loop_skip_;         // loop-closing SearchByProjection: the skip flags
    // SearchBySim3 / SearchByBoW(KF, KF): the per-feature masks and the index-valued matches
    std::vector<uint8_t> sim3_search1_, sim3_search2_;
    std::vector<int> sim3_m12_;
};

// A DBoW2::BowVector (std::map<WordId, WordValue>) as two parallel arrays, word ids ascending —
// what orbfe_bow_transform writes.
struct BowVector {
    std::vector<int32_t> ids;
    std::vector<double> values;
};

// ORB_SLAM2::ORBVocabulary (ORBVocabulary.h:31-32, DBoW2 TemplatedVocabulary<FORB>) held on the GPU.
class ORBVocabulary {
public:
    // loadFromTextFile (TemplatedVocabulary.h:1351-1436)
    explicit ORBVocabulary(const std::string& path, int device = 0) {
        int st = ORBFE_OK;
        v_ = orbfe_vocabulary_load_text(path.c_str(), device, &st);
        if (!v_) throw Error("orbfe_vocabulary_load_text", st);
    }
    ~ORBVocabulary() { orbfe_vocabulary_destroy(v_); }
    ORBVocabulary(const ORBVocabulary&) = delete;
    ORBVocabulary& operator=(const ORBVocabulary&) = delete;

    // size() (TemplatedVocabulary.h:122): the number of words
    int size() const {
        int32_t info[6];
        check("orbfe_vocabulary_info", orbfe_vocabulary_info(v_, info));
        return info[5];
    }
    // score(v1, v2) (TemplatedVocabulary.h -> ScoringObject.cpp:23-311)
    double score(const BowVector& v1, const BowVector& v2) const {
        double s = 0.0;
        check("orbfe_vocabulary_score",
              orbfe_vocabulary_score(v_, v1.ids.data(), v1.values.data(), (int)v1.ids.size(),
                                     v2.ids.data(), v2.values.data(), (int)v2.ids.size(), &s));
        return s;
    }
    orbfe_vocabulary* handle() const { return v_; }

private:
    orbfe_vocabulary* v_ = nullptr;
};

// ORB_SLAM2::KeyFrameDatabase (KeyFrameDatabase.h:48-94) keyed by the caller's keyframe ids
// (KeyFrame::mnId); it holds the id <-> slot map of the device database.
class KeyFrameDatabase {
public:
    explicit KeyFrameDatabase(const ORBVocabulary& voc, int cap = 4096, int slots_hint = 0) {
        int st = ORBFE_OK;
        db_ = orbfe_kfdb_create(voc.handle(), cap, slots_hint, &st);
        if (!db_) throw Error("orbfe_kfdb_create", st);
    }
    ~KeyFrameDatabase() { orbfe_kfdb_destroy(db_); }
    KeyFrameDatabase(const KeyFrameDatabase&) = delete;
    KeyFrameDatabase& operator=(const KeyFrameDatabase&) = delete;

    // add(pKF) (KeyFrameDatabase.cc:115-121).  An id already present throws
    // Error(ORBFE_ERR_UNSUPPORTED): the reference would list the keyframe twice in every word's
    // list and count its words double.
    void add(uint64_t mnId, const BowVector& bow) {
        if (slot_of(mnId) >= 0) throw Error("KeyFrameDatabase::add", ORBFE_ERR_UNSUPPORTED);
        int32_t slot = -1;
        check("orbfe_kfdb_add", orbfe_kfdb_add(db_, bow.ids.data(), bow.values.data(),
                                               (int)bow.ids.size(), &slot));
        if ((size_t)slot >= id_.size()) id_.resize((size_t)slot + 1, 0);
        id_[slot] = mnId;
        slot_[mnId] = slot;
    }
    // erase(pKF) (KeyFrameDatabase.cc:123-142); an unknown id is ignored, as there.
    void erase(uint64_t mnId) {
        const int slot = slot_of(mnId);
        if (slot < 0) return;
        check("orbfe_kfdb_erase", orbfe_kfdb_erase(db_, slot));
        slot_.erase(mnId);
    }
    void clear() {  // KeyFrameDatabase.cc:144-148
        check("orbfe_kfdb_clear", orbfe_kfdb_clear(db_));
        slot_.clear();
    }
    // pKF->GetBestCovisibilityKeyFrames(10) (KeyFrame.cc:895-903) as ids, at most 10, in its
    // order; ids that are not in the database keep their place and are skipped.  The ids are
    // resolved to slots now: a neighbour that enters the database later is not seen until the
    // list is set again (an erased one leaves every list by itself).
    void SetBestCovisibilityKeyFrames(uint64_t mnId, const std::vector<uint64_t>& neighbours) {
        const int slot = slot_of(mnId);
        if (slot < 0 || neighbours.size() > 10)
            throw Error("KeyFrameDatabase::SetBestCovisibilityKeyFrames", ORBFE_ERR_ARG);
        int32_t n[10];
        for (size_t i = 0; i < neighbours.size(); ++i) n[i] = slot_of(neighbours[i]);
        check("orbfe_kfdb_set_covisibility",
              orbfe_kfdb_set_covisibility(db_, slot, (int)neighbours.size(), n));
    }
    // DetectLoopCandidates(pKF, minScore) (KeyFrameDatabase.cc:151-272): mnId, mBowVec and
    // GetConnectedKeyFrames() of pKF.  Returns vpLoopCandidates as ids.  `uninitialised` (may be
    // null) is set when the reference would have read a score it never wrote.
    std::vector<uint64_t> DetectLoopCandidates(uint64_t mnId, const BowVector& bow,
                                               const std::vector<uint64_t>& connected,
                                               float minScore, bool* uninitialised = nullptr) {
        std::vector<int32_t> conn;
        for (uint64_t c : connected) {
            const int s = slot_of(c);
            if (s >= 0) conn.push_back(s);
        }
        std::vector<int32_t> cand(std::max<size_t>(id_.size(), 1));
        int32_t n = 0;
        const int st = orbfe_kfdb_detect_loop_candidates(
            db_, mnId, bow.ids.data(), bow.values.data(), (int)bow.ids.size(), (int)conn.size(),
            conn.data(), minScore, cand.data(), (int)cand.size(), &n);
        return result("orbfe_kfdb_detect_loop_candidates", st, cand, n, uninitialised);
    }
    // DetectRelocalizationCandidates(F) (KeyFrameDatabase.cc:274-389): mnId and mBowVec of F.
    std::vector<uint64_t> DetectRelocalizationCandidates(uint64_t mnId, const BowVector& bow,
                                                         bool* uninitialised = nullptr) {
        std::vector<int32_t> cand(std::max<size_t>(id_.size(), 1));
        int32_t n = 0;
        const int st = orbfe_kfdb_detect_relocalization_candidates(
            db_, mnId, bow.ids.data(), bow.values.data(), (int)bow.ids.size(), cand.data(),
            (int)cand.size(), &n);
        return result("orbfe_kfdb_detect_relocalization_candidates", st, cand, n, uninitialised);
    }
    orbfe_kfdb* handle() const { return db_; }

private:
    int slot_of(uint64_t mnId) const {
        const auto it = slot_.find(mnId);
        return it == slot_.end() ? -1 : it->second;
    }
    std::vector<uint64_t> result(const char* fn, int st, const std::vector<int32_t>& cand, int n,
                                 bool* uninitialised) const {
        if (st != ORBFE_OK && st != ORBFE_ERR_UNSUPPORTED) throw Error(fn, st);
        if (uninitialised) *uninitialised = st == ORBFE_ERR_UNSUPPORTED;
        std::vector<uint64_t> out;
        for (int i = 0; i < n; ++i) out.push_back(id_[cand[i]]);
        return out;
    }
    orbfe_kfdb* db_ = nullptr;
    std::vector<uint64_t> id_;                 // slot -> mnId
    std::unordered_map<uint64_t, int> slot_;   // mnId -> slot, the keyframes in the database
};

// Tracking::UpdateLocalMap (Tracking.cc:1455-1599) over the device mirror of the map graph
// (orbfe_map), keyed by the caller's KeyFrame::mnId and MapPoint::mnId.  The mutators carry the
// names of the reference methods whose effect they mirror; call them from those methods
// (INTEGRATION.md §3h).  Every keyframe is added with order_key = (uintptr_t)pKF: the reference
// iterates map<KeyFrame*, int> and set<KeyFrame*> in address order.
class LocalMap {
public:
    static constexpr uint64_t kNone = ~0ull;  // a NULL MapPoint* / KeyFrame*

    struct Result {
        std::vector<uint64_t> mvpLocalKeyFrames;   // mnIds, in the reference's order
        std::vector<uint64_t> mvpLocalMapPoints;
        uint64_t mpReferenceKF = kNone;
    };

    explicit LocalMap(int device = 0, int keyframes_hint = 0, int points_hint = 0) {
        int st = ORBFE_OK;
        m_ = orbfe_map_create(device, keyframes_hint, points_hint, &st);
        if (!m_) throw Error("orbfe_map_create", st);
    }
    ~LocalMap() { orbfe_map_destroy(m_); }
    LocalMap(const LocalMap&) = delete;
    LocalMap& operator=(const LocalMap&) = delete;

    void clear() {  // Tracking::Reset
        check("orbfe_map_clear", orbfe_map_clear(m_));
        kf_id_.clear();
        mp_id_.clear();
        kf_slot_.clear();
        mp_slot_.clear();
        children_.clear();
    }
    // new MapPoint(...)
    void NewMapPoint(uint64_t mpId) {
        if (mp_slot_.count(mpId)) throw Error("LocalMap::NewMapPoint", ORBFE_ERR_ARG);
        int32_t s = -1;
        check("orbfe_map_add_points", orbfe_map_add_points(m_, 1, &s));
        mp_id_.push_back(mpId);
        mp_slot_[mpId] = s;
    }
    // new KeyFrame(F, ...): pKF's address as the order key, mvpMapPoints as point ids or kNone
    void NewKeyFrame(uint64_t kfId, uint64_t order_key, const std::vector<uint64_t>& mvpMapPoints) {
        if (kf_slot_.count(kfId)) throw Error("LocalMap::NewKeyFrame", ORBFE_ERR_ARG);
        std::vector<int32_t> mps(mvpMapPoints.size());
        for (size_t i = 0; i < mps.size(); ++i) mps[i] = mp(mvpMapPoints[i], true);
        int32_t s = -1;
        check("orbfe_map_add_keyframe",
              orbfe_map_add_keyframe(m_, order_key, (int)mps.size(), mps.data(), &s));
        kf_id_.push_back(kfId);
        kf_slot_[kfId] = s;
    }
    // KeyFrame::AddMapPoint(pMP, idx); mpId = kNone: EraseMapPointMatch(idx)
    void AddMapPoint(uint64_t kfId, size_t idx, uint64_t mpId) {
        const int32_t p = mp(mpId, true);
        check("orbfe_map_set_keyframe_points", orbfe_map_set_keyframe_points(m_, kf(kfId), (int)idx, 1, &p));
    }
    // MapPoint::AddObservation(pKF, idx) / EraseObservation(pKF)
    void AddObservation(uint64_t mpId, uint64_t kfId) {
        const int32_t p = mp(mpId), k = kf(kfId);
        check("orbfe_map_add_observations", orbfe_map_add_observations(m_, 1, &p, &k));
    }
    void EraseObservation(uint64_t mpId, uint64_t kfId) {
        const int32_t p = mp(mpId), k = kf(kfId);
        check("orbfe_map_erase_observations", orbfe_map_erase_observations(m_, 1, &p, &k));
    }
    // MapPoint::SetBadFlag / KeyFrame::SetBadFlag (mbBad alone: the observations and the
    // connections change through their own hooks)
    void SetBadFlag(uint64_t mpId) {
        const int32_t p = mp(mpId);
        check("orbfe_map_set_points_bad", orbfe_map_set_points_bad(m_, 1, &p, 1));
    }
    void SetKeyFrameBadFlag(uint64_t kfId) {
        check("orbfe_map_set_keyframe_bad", orbfe_map_set_keyframe_bad(m_, kf(kfId), 1));
    }
    // KeyFrame::UpdateBestCovisibles: the first 10 of mvpOrderedConnectedKeyFrames; an id the
    // mirror does not hold keeps its place and is skipped
    void UpdateBestCovisibles(uint64_t kfId, const std::vector<uint64_t>& ordered) {
        int32_t n[10];
        const int cnt = (int)std::min<size_t>(ordered.size(), 10);
        for (int i = 0; i < cnt; ++i) {
            const auto it = kf_slot_.find(ordered[i]);
            n[i] = it == kf_slot_.end() ? -1 : it->second;
        }
        check("orbfe_map_set_covisibility", orbfe_map_set_covisibility(m_, kf(kfId), cnt, n));
    }
    // KeyFrame::AddChild / EraseChild / ChangeParent (KeyFrame.cc:441-458)
    void AddChild(uint64_t kfId, uint64_t childId) {
        std::vector<int32_t>& c = children_[kf(kfId)];
        const int32_t s = kf(childId);
        if (std::find(c.begin(), c.end(), s) == c.end()) c.push_back(s);
        check("orbfe_map_set_children", orbfe_map_set_children(m_, kf(kfId), (int)c.size(), c.data()));
    }
    void EraseChild(uint64_t kfId, uint64_t childId) {
        std::vector<int32_t>& c = children_[kf(kfId)];
        c.erase(std::remove(c.begin(), c.end(), kf(childId)), c.end());
        check("orbfe_map_set_children", orbfe_map_set_children(m_, kf(kfId), (int)c.size(), c.data()));
    }
    void ChangeParent(uint64_t kfId, uint64_t parentId) {
        check("orbfe_map_set_parent", orbfe_map_set_parent(m_, kf(kfId), kf(parentId)));
        AddChild(parentId, kfId);
    }
    // mpParent alone (a keyframe loaded from a map archive; kNone: no parent)
    void SetParent(uint64_t kfId, uint64_t parentId) {
        check("orbfe_map_set_parent",
              orbfe_map_set_parent(m_, kf(kfId), parentId == kNone ? -1 : kf(parentId)));
    }
    // mvpLocalKeyFrames / mpReferenceKF assigned directly (Tracking.cc:789, :969-970)
    void SetLocalKeyFrames(const std::vector<uint64_t>& kfIds, uint64_t refId) {
        std::vector<int32_t> s;
        for (uint64_t id : kfIds) s.push_back(kf(id));
        check("orbfe_map_set_local_keyframes",
              orbfe_map_set_local_keyframes(m_, (int)s.size(), s.data(), refId == kNone ? -1 : kf(refId)));
    }
    // UpdateLocalMap() with mCurrentFrame.mnId = frameId; mvpMapPoints holds point ids or kNone
    // and gets the bad ones set to kNone (:1508)
    Result UpdateLocalMap(uint64_t frameId, std::vector<uint64_t>& mvpMapPoints) {
        std::vector<int32_t> f(mvpMapPoints.size());
        for (size_t i = 0; i < f.size(); ++i) f[i] = mp(mvpMapPoints[i], true);
        std::vector<int32_t> kfs(ORBFE_MAP_MAX_VOTED + 8), pts(std::max<size_t>(mp_id_.size(), 1));
        int32_t nk = 0, ref = -1, np = 0;
        check("orbfe_map_update_local",
              orbfe_map_update_local(m_, frameId, (int)f.size(), f.data(), kfs.data(), (int)kfs.size(),
                                     &nk, &ref, pts.data(), (int)pts.size(), &np));
        Result r;
        for (int i = 0; i < nk; ++i) r.mvpLocalKeyFrames.push_back(kf_id_[kfs[i]]);
        for (int i = 0; i < np; ++i) r.mvpLocalMapPoints.push_back(mp_id_[pts[i]]);
        if (ref >= 0) r.mpReferenceKF = kf_id_[ref];
        for (size_t i = 0; i < f.size(); ++i)
            if (f[i] < 0) mvpMapPoints[i] = kNone;
        return r;
    }
    // ---- the covisibility graph on the device
    // KeyFrame::UpdateConnections (KeyFrame.cc:1010-1100) of one keyframe, or of several in that
    // order (System.cc:188-191 after LoadMap: every keyframe of the map); `mnId != 0` is kfId != 0.
    // The children the device assigned are added to the cache AddChild / EraseChild upload from.
    void UpdateConnections(uint64_t kfId) { UpdateConnections(std::vector<uint64_t>{kfId}); }
    void UpdateConnections(const std::vector<uint64_t>& kfIds) {
        std::vector<int32_t> s, parent(kfIds.size(), -1);
        std::vector<uint8_t> allow;
        for (uint64_t id : kfIds) {
            s.push_back(kf(id));
            allow.push_back(id != 0);
        }
        check("orbfe_map_update_connections",
              orbfe_map_update_connections(m_, (int)s.size(), s.data(), allow.data(), parent.data(), nullptr));
        for (size_t i = 0; i < s.size(); ++i) {
            if (parent[i] < 0) continue;
            std::vector<int32_t>& c = children_[parent[i]];
            if (std::find(c.begin(), c.end(), s[i]) == c.end()) c.push_back(s[i]);
        }
    }
    // KeyFrame::AddConnection / EraseConnection / UpdateBestCovisibles (:844-878, :1295-1309)
    void AddConnection(uint64_t kfId, uint64_t otherId, int weight) {
        check("orbfe_map_add_connection", orbfe_map_add_connection(m_, kf(kfId), kf(otherId), weight));
    }
    void EraseConnection(uint64_t kfId, uint64_t otherId) {
        check("orbfe_map_erase_connection", orbfe_map_erase_connection(m_, kf(kfId), kf(otherId)));
    }
    void UpdateBestCovisibles(uint64_t kfId) {
        check("orbfe_map_update_best_covisibles", orbfe_map_update_best_covisibles(m_, kf(kfId)));
    }
    // the connection part of KeyFrame::SetBadFlag (:1188-1189, :1198-1199)
    void EraseKeyFrameConnections(uint64_t kfId) {
        check("orbfe_map_erase_keyframe_connections", orbfe_map_erase_keyframe_connections(m_, kf(kfId)));
    }
    void SetFirstConnection(uint64_t kfId, bool flag) {
        check("orbfe_map_set_first_connection", orbfe_map_set_first_connection(m_, kf(kfId), flag));
    }
    // GetConnectedKeyFrames (:880-887) in pointer order; GetVectorCovisibleKeyFrames (:889-893);
    // GetBestCovisibilityKeyFrames (:895-903)
    std::vector<uint64_t> GetConnectedKeyFrames(uint64_t kfId) { return ids(row(kfId, false).first); }
    std::vector<uint64_t> GetVectorCovisibleKeyFrames(uint64_t kfId) { return ids(row(kfId, true).first); }
    std::vector<uint64_t> GetBestCovisibilityKeyFrames(uint64_t kfId, int N) {
        std::vector<uint64_t> v = GetVectorCovisibleKeyFrames(kfId);
        if ((int)v.size() >= N) v.resize((size_t)std::max(N, 0));
        return v;
    }
    // mvOrderedWeights, next to GetVectorCovisibleKeyFrames
    std::vector<int> GetOrderedWeights(uint64_t kfId) { return row(kfId, true).second; }
    // GetCovisiblesByWeight (:905-920): upper_bound with a > b over the descending weights; when
    // every weight is >= w the iterator is end() and the reference returns nothing
    std::vector<uint64_t> GetCovisiblesByWeight(uint64_t kfId, int w) {
        const auto r = row(kfId, true);
        const auto it = std::upper_bound(r.second.begin(), r.second.end(), w, [](int a, int b) { return a > b; });
        if (r.first.empty() || it == r.second.end()) return {};
        return ids(std::vector<int32_t>(r.first.begin(), r.first.begin() + (it - r.second.begin())));
    }
    // GetWeight (:922-929)
    int GetWeight(uint64_t kfId, uint64_t otherId) {
        const auto r = row(kfId, false);
        const auto it = std::find(r.first.begin(), r.first.end(), kf(otherId));
        return it == r.first.end() ? 0 : r.second[(size_t)(it - r.first.begin())];
    }
    // GetParent (kNone: none) / GetChilds in pointer order / mbFirstConnection
    uint64_t GetParent(uint64_t kfId) { return tree(kfId).parent; }
    std::vector<uint64_t> GetChilds(uint64_t kfId) { return tree(kfId).children; }
    bool FirstConnection(uint64_t kfId) { return tree(kfId).first; }

    // ---- culling on the device
    struct BadFlagResult {
        int what = ORBFE_MAP_BAD_NOTHING;                           // ORBFE_MAP_BAD_*
        std::vector<uint64_t> bad_points;                           // MapPoint::SetBadFlag ran, in order
        std::vector<std::pair<uint64_t, uint64_t>> reparented;      // (child, new parent), in order
    };
    struct CullingResult {
        std::vector<uint64_t> listed;                               // vpLocalKeyFrames
        std::vector<int> result;                                    // ORBFE_MAP_CULL_* per listed keyframe
        std::vector<uint64_t> culled;                               // SetBadFlag ran, in order
        std::vector<uint64_t> bad_points;
        std::vector<std::pair<uint64_t, uint64_t>> reparented;
    };
    // mvKeysUn[i].octave, mvuRight, mvDepth (empty: all 0 / -1 / -1) and mThDepth of a keyframe
    void SetKeyFrameFeatures(uint64_t kfId, const std::vector<int32_t>& octaves, const std::vector<float>& mvuRight,
                             const std::vector<float>& mvDepth, float mThDepth) {
        const size_t n = std::max(octaves.size(), std::max(mvuRight.size(), mvDepth.size()));
        check("orbfe_map_set_keyframe_features",
              orbfe_map_set_keyframe_features(m_, kf(kfId), (int)n, octaves.empty() ? nullptr : octaves.data(),
                                              mvuRight.empty() ? nullptr : mvuRight.data(),
                                              mvDepth.empty() ? nullptr : mvDepth.data(), mThDepth));
    }
    // MapPoint::AddObservation(pKF, idx) in full (MapPoint.cc:339-350)
    void AddObservation(uint64_t mpId, uint64_t kfId, size_t idx) {
        const int32_t p = mp(mpId), k = kf(kfId), x = (int32_t)idx;
        check("orbfe_map_add_observations_idx", orbfe_map_add_observations_idx(m_, 1, &p, &k, &x));
    }
    // MapPoint::EraseObservation(pKF) in full (:352-378): *went_bad when nObs <= 2 set the point bad
    void EraseObservation(uint64_t mpId, uint64_t kfId, bool* went_bad) {
        int32_t b = 0;
        check("orbfe_map_erase_observation", orbfe_map_erase_observation(m_, mp(mpId), kf(kfId), &b));
        if (went_bad) *went_bad = b != 0;
    }
    // MapPoint::SetBadFlag in full (:392-409)
    void SetMapPointBadFlag(uint64_t mpId) {
        const int32_t p = mp(mpId);
        check("orbfe_map_set_point_bad_flag", orbfe_map_set_point_bad_flag(m_, 1, &p));
    }
    // mbBad of a keyframe alone: what SetKeyFrameBadFlag(kfId) without a second argument does
    void set_keyframe_bad(uint64_t kfId) { SetKeyFrameBadFlag(kfId); }
    // KeyFrame::SetBadFlag in full (KeyFrame.cc:1174-1287); is_first is `mnId == 0`
    BadFlagResult SetKeyFrameBadFlag(uint64_t kfId, bool is_first) {
        return bad_flag([&](int32_t* what, int32_t* bad, int nb_cap, int32_t* nb, int32_t* pr, int np_cap, int32_t* np) {
            return orbfe_map_set_keyframe_bad_flag(m_, kf(kfId), is_first, what, bad, nb_cap, nb, pr, np_cap, np);
        }, "orbfe_map_set_keyframe_bad_flag");
    }
    void SetNotErase(uint64_t kfId) { check("orbfe_map_set_not_erase", orbfe_map_set_not_erase(m_, kf(kfId), 1)); }
    // KeyFrame::SetErase (:1158-1172); has_loop_edges is `!mspLoopEdges.empty()`
    BadFlagResult SetErase(uint64_t kfId, bool has_loop_edges, bool is_first = false) {
        return bad_flag([&](int32_t* what, int32_t* bad, int nb_cap, int32_t* nb, int32_t* pr, int np_cap, int32_t* np) {
            return orbfe_map_set_erase(m_, kf(kfId), has_loop_edges, is_first, what, bad, nb_cap, nb, pr, np_cap, np);
        }, "orbfe_map_set_erase");
    }
    bool NotErase(uint64_t kfId) { return erase_flags(kfId).first; }
    bool ToBeErased(uint64_t kfId) { return erase_flags(kfId).second; }
    void IncreaseFound(uint64_t mpId, int n = 1) { increase(ORBFE_MAP_FOUND, mpId, n); }
    void IncreaseVisible(uint64_t mpId, int n = 1) { increase(ORBFE_MAP_VISIBLE, mpId, n); }
    void SetFirstKFid(uint64_t mpId, int64_t id) {
        const int32_t p = mp(mpId);
        check("orbfe_map_set_point_counters", orbfe_map_set_point_counters(m_, 1, &p, nullptr, nullptr, nullptr, &id));
    }
    int Observations(uint64_t mpId) { return counters(mpId)[0]; }
    float GetFoundRatio(uint64_t mpId) {
        const auto c = counters(mpId);
        return static_cast<float>(c[1]) / c[2];
    }
    bool MapPointIsBad(uint64_t mpId) { return bad(ORBFE_MAP_POINTS, mp(mpId)); }
    bool KeyFrameIsBad(uint64_t kfId) { return bad(ORBFE_MAP_KEYFRAMES, kf(kfId)); }
    // GetMapPointMatches as ids or kNone; GetObservations as (keyframe id, idx) in slot order
    std::vector<uint64_t> GetMapPointMatches(uint64_t kfId) {
        std::vector<int32_t> s(ORBFE_MAP_MAX_KF_SLOTS);
        int32_t n = 0;
        check("orbfe_map_get_keyframe_points", orbfe_map_get_keyframe_points(m_, kf(kfId), s.data(), (int)s.size(), &n));
        std::vector<uint64_t> out((size_t)n, kNone);
        for (int i = 0; i < n; ++i)
            if (s[i] >= 0) out[i] = mp_id_[s[i]];
        return out;
    }
    std::vector<std::pair<uint64_t, int64_t>> GetObservations(uint64_t mpId) {
        std::vector<int32_t> k(std::max<size_t>(kf_id_.size(), 1)), x(k.size());
        int32_t n = 0;
        check("orbfe_map_get_observations", orbfe_map_get_observations(m_, mp(mpId), k.data(), x.data(), (int)k.size(), &n));
        std::vector<std::pair<uint64_t, int64_t>> out;
        for (int i = 0; i < n; ++i) out.push_back({kf_id_[k[i]], x[i]});
        return out;
    }
    // KeyFrame::TrackedMapPoints(minObs) (KeyFrame.cc:971-996)
    int TrackedMapPoints(uint64_t kfId, int minObs) {
        int32_t n = 0;
        check("orbfe_map_tracked_map_points", orbfe_map_tracked_map_points(m_, kf(kfId), minObs, &n));
        return n;
    }
    // LocalMapping::MapPointCulling (LocalMapping.cc:170-205): mlpRecentAddedMapPoints is edited in
    // place; returns the points whose SetBadFlag ran
    std::vector<uint64_t> MapPointCulling(std::list<uint64_t>& mlpRecentAddedMapPoints, uint64_t nCurrentKFid,
                                          bool mbMonocular) {
        std::vector<int32_t> l, gone(std::max<size_t>(mlpRecentAddedMapPoints.size(), 1));
        for (uint64_t id : mlpRecentAddedMapPoints) l.push_back(mp(id));
        int32_t n = 0, nc = 0;
        check("orbfe_map_cull_points", orbfe_map_cull_points(m_, (int64_t)nCurrentKFid, mbMonocular, l.data(),
                                                             (int)l.size(), &n, gone.data(), &nc));
        mlpRecentAddedMapPoints.clear();
        for (int i = 0; i < n; ++i) mlpRecentAddedMapPoints.push_back(mp_id_[l[i]]);
        std::vector<uint64_t> out;
        for (int i = 0; i < nc; ++i) out.push_back(mp_id_[gone[i]]);
        return out;
    }
    // LocalMapping::KeyFrameCulling (:632-698) over GetVectorCovisibleKeyFrames of the current
    // keyframe; the keyframe with id 0 is the map's first
    CullingResult KeyFrameCulling(uint64_t currentKfId, bool mbMonocular) {
        const auto first = kf_slot_.find(0);
        std::vector<int32_t> res(ORBFE_MAP_MAX_CULL_LIST), bad(std::max<size_t>(mp_id_.size(), 1));
        std::vector<int32_t> pr(2 * std::max<size_t>(kf_id_.size(), 1) * 8);
        const std::vector<uint64_t> listed = GetVectorCovisibleKeyFrames(currentKfId);
        pr.resize(2 * std::max<size_t>(kf_id_.size(), 1) * std::max<size_t>(listed.size(), 1));
        int32_t nl = 0, nb = 0, np = 0;
        check("orbfe_map_cull_keyframes",
              orbfe_map_cull_keyframes(m_, kf(currentKfId), -1, nullptr, first == kf_slot_.end() ? -1 : first->second,
                                       mbMonocular, res.data(), (int)res.size(), &nl, bad.data(), (int)bad.size(), &nb,
                                       pr.data(), (int)pr.size() / 2, &np));
        CullingResult r;
        r.listed = listed;
        r.result.assign(res.begin(), res.begin() + nl);
        for (int i = 0; i < nl; ++i)
            if (res[i] == ORBFE_MAP_CULL_CULLED) r.culled.push_back(listed[(size_t)i]);
        for (int i = 0; i < nb; ++i) r.bad_points.push_back(mp_id_[bad[i]]);
        for (int i = 0; i < np; ++i) r.reparented.push_back({kf_id_[pr[2 * i]], kf_id_[pr[2 * i + 1]]});
        refresh_children();
        return r;
    }

    // mnTrackReferenceForFrame of a keyframe / a point
    uint64_t KeyFrameStamp(uint64_t kfId) { return stamp(ORBFE_MAP_KEYFRAMES, kf(kfId)); }
    uint64_t MapPointStamp(uint64_t mpId) { return stamp(ORBFE_MAP_POINTS, mp(mpId)); }
    orbfe_map* handle() const { return m_; }

    // ---- MapPoint refresh (MapPoint.cc:483-548, 571-619; LocalMapping.cc:140-161).  `arrays` are
    // the caller's map-wide device arrays, indexed by MapPointSlot(mnId): xyz is read; normal,
    // min_dist, max_dist and desc are written.
    int32_t MapPointSlot(uint64_t mpId) const { return mp(mpId); }
    // mvScaleFactors of the map's keyframes
    void SetScaleFactors(const std::vector<float>& mvScaleFactors) {
        check("orbfe_map_set_scale_factors",
              orbfe_map_set_scale_factors(m_, (int)mvScaleFactors.size(), mvScaleFactors.data()));
    }
    // pKF->GetCameraCenter(), after every SetPose
    void SetCameraCenter(uint64_t kfId, const float Ow[3]) {
        const int32_t s = kf(kfId);
        check("orbfe_map_set_keyframe_centers", orbfe_map_set_keyframe_centers(m_, 1, &s, Ow));
    }
    // pKF->mDescriptors: n rows of 32 bytes, n = the keyframe's keypoints; on the host or on the device
    void SetDescriptors(uint64_t kfId, const uint8_t* mDescriptors, size_t n) {
        check("orbfe_map_set_keyframe_descriptors",
              orbfe_map_set_keyframe_descriptors(m_, kf(kfId), (int)n, mDescriptors));
    }
    void SetDescriptorsDevice(uint64_t kfId, const uint8_t* d_desc, size_t n) {
        check("orbfe_map_set_keyframe_descriptors_device",
              orbfe_map_set_keyframe_descriptors_device(m_, kf(kfId), (int)n, d_desc));
    }
    // mpRefKF (kNone: NULL); the handle keeps it through every EraseObservation from here on
    void SetReferenceKeyFrame(uint64_t mpId, uint64_t kfId) {
        const int32_t p = mp(mpId), k = kfId == kNone ? -1 : kf(kfId);
        check("orbfe_map_set_point_ref_keyframes", orbfe_map_set_point_ref_keyframes(m_, 1, &p, &k));
    }
    uint64_t GetReferenceKeyFrame(uint64_t mpId) {
        const int32_t p = mp(mpId);
        int32_t k = -1;
        check("orbfe_map_get_point_ref_keyframes", orbfe_map_get_point_ref_keyframes(m_, 1, &p, &k));
        return k < 0 ? kNone : kf_id_[k];
    }
    // Both functions (by the bits of `what`) of the listed points -> per point the bits of what was
    // written; ORBFE_MAP_REFRESH_UNSUPPORTED marks a point whose normal and distances were left
    // alone because the reference reads out of range there (everything else was written).
    std::vector<uint8_t> RefreshPoints(const std::vector<uint64_t>& mpIds, int what,
                                       const orbfe_map_point_arrays& arrays) {
        std::vector<int32_t> s(mpIds.size());
        for (size_t i = 0; i < s.size(); ++i) s[i] = mp(mpIds[i], true);
        std::vector<uint8_t> res(mpIds.size(), 0);
        const int st = orbfe_map_refresh_points(m_, what, (int)s.size(), s.data(), &arrays, res.data());
        if (st != ORBFE_OK && st != ORBFE_ERR_UNSUPPORTED) throw Error("orbfe_map_refresh_points", st);
        return res;
    }
    // pMP->UpdateNormalAndDepth() / pMP->ComputeDistinctiveDescriptors(); the second alone is the
    // last line of MapPoint::Replace (MapPoint.cc:453)
    uint8_t UpdateNormalAndDepth(uint64_t mpId, const orbfe_map_point_arrays& arrays) {
        return RefreshPoints({mpId}, ORBFE_MAP_REFRESH_NORMAL_DEPTH, arrays)[0];
    }
    uint8_t ComputeDistinctiveDescriptors(uint64_t mpId, const orbfe_map_point_arrays& arrays) {
        return RefreshPoints({mpId}, ORBFE_MAP_REFRESH_DESCRIPTOR, arrays)[0];
    }
    // The loop at LocalMapping.cc:518-530 over pKF's mvpMapPoints where they lie -> the entries refreshed
    int RefreshKeyFramePoints(uint64_t kfId, const orbfe_map_point_arrays& arrays,
                              int what = ORBFE_MAP_REFRESH_NORMAL_DEPTH | ORBFE_MAP_REFRESH_DESCRIPTOR) {
        int32_t n = 0;
        const int st = orbfe_map_refresh_keyframe_points(m_, kf(kfId), what, &arrays, &n);
        if (st != ORBFE_OK && st != ORBFE_ERR_UNSUPPORTED) throw Error("orbfe_map_refresh_keyframe_points", st);
        return n;
    }
    // The map-point loop of LocalMapping::ProcessNewKeyFrame -> what it appends to mlpRecentAddedMapPoints
    std::vector<uint64_t> ProcessNewKeyFrame(uint64_t kfId, const orbfe_map_point_arrays& arrays) {
        std::vector<int32_t> rec(ORBFE_MAP_MAX_KF_SLOTS);
        int32_t n = 0;
        const int st = orbfe_map_process_new_keyframe(m_, kf(kfId), &arrays, rec.data(), (int)rec.size(), &n);
        if (st != ORBFE_OK && st != ORBFE_ERR_UNSUPPORTED) throw Error("orbfe_map_process_new_keyframe", st);
        std::vector<uint64_t> out;
        for (int i = 0; i < n; ++i) out.push_back(mp_id_[rec[i]]);
        return out;
    }

private:
    int32_t kf(uint64_t id) const {
        const auto it = kf_slot_.find(id);
        if (it == kf_slot_.end()) throw Error("LocalMap: unknown keyframe", ORBFE_ERR_ARG);
        return it->second;
    }
    int32_t mp(uint64_t id, bool none_ok = false) const {
        if (none_ok && id == kNone) return -1;
        const auto it = mp_slot_.find(id);
        if (it == mp_slot_.end()) throw Error("LocalMap: unknown map point", ORBFE_ERR_ARG);
        return it->second;
    }
    template <class F>
    BadFlagResult bad_flag(F&& call, const char* fn) {
        std::vector<int32_t> bad(std::max<size_t>(mp_id_.size(), 1)), pr(2 * std::max<size_t>(kf_id_.size(), 1));
        int32_t what = 0, nb = 0, np = 0;
        check(fn, call(&what, bad.data(), (int)bad.size(), &nb, pr.data(), (int)pr.size() / 2, &np));
        BadFlagResult r;
        r.what = what;
        for (int i = 0; i < nb; ++i) r.bad_points.push_back(mp_id_[bad[i]]);
        for (int i = 0; i < np; ++i) r.reparented.push_back({kf_id_[pr[2 * i]], kf_id_[pr[2 * i + 1]]});
        if (what == ORBFE_MAP_BAD_DONE) refresh_children();
        return r;
    }
    // the cache AddChild / EraseChild upload from, read back after the device changed the tree
    void refresh_children() {
        std::vector<int32_t> c(std::max<size_t>(kf_id_.size(), 1));
        for (size_t s = 0; s < kf_id_.size(); ++s) {
            int32_t n = 0;
            check("orbfe_map_get_spanning_tree",
                  orbfe_map_get_spanning_tree(m_, (int)s, nullptr, nullptr, c.data(), (int)c.size(), &n));
            if (n || children_.count((int32_t)s)) children_[(int32_t)s].assign(c.begin(), c.begin() + n);
        }
    }
    std::pair<bool, bool> erase_flags(uint64_t kfId) {
        int32_t a = 0, b = 0;
        check("orbfe_map_get_erase_flags", orbfe_map_get_erase_flags(m_, kf(kfId), &a, &b));
        return {a != 0, b != 0};
    }
    void increase(int kind, uint64_t mpId, int n) {
        const int32_t p = mp(mpId), a = n;
        check("orbfe_map_increase_counters", orbfe_map_increase_counters(m_, kind, 1, &p, &a));
    }
    std::array<int32_t, 3> counters(uint64_t mpId) {
        const int32_t p = mp(mpId);
        std::array<int32_t, 3> c{};
        check("orbfe_map_get_point_counters", orbfe_map_get_point_counters(m_, 1, &p, &c[0], &c[1], &c[2], nullptr));
        return c;
    }
    bool bad(int kind, int32_t slot) {
        uint8_t b = 0;
        check("orbfe_map_get_bad_flags", orbfe_map_get_bad_flags(m_, kind, 1, &slot, &b));
        return b != 0;
    }
    uint64_t stamp(int kind, int32_t slot) {
        uint64_t v = 0;
        check("orbfe_map_get_stamps", orbfe_map_get_stamps(m_, kind, 1, &slot, &v));
        return v;
    }
    std::vector<uint64_t> ids(const std::vector<int32_t>& slots) const {
        std::vector<uint64_t> out;
        for (int32_t s : slots) out.push_back(kf_id_[s]);
        return out;
    }
    // the weight map (pointer order) or the ordered list of a keyframe: (slots, weights)
    std::pair<std::vector<int32_t>, std::vector<int>> row(uint64_t kfId, bool ordered) {
        std::vector<int32_t> s(ORBFE_MAP_MAX_VOTED), w(ORBFE_MAP_MAX_VOTED);
        int32_t n = 0;
        if (ordered)
            check("orbfe_map_get_ordered_connections",
                  orbfe_map_get_ordered_connections(m_, kf(kfId), s.data(), w.data(), (int)s.size(), &n));
        else
            check("orbfe_map_get_connections",
                  orbfe_map_get_connections(m_, kf(kfId), s.data(), w.data(), (int)s.size(), &n));
        s.resize((size_t)n);
        return {s, std::vector<int>(w.begin(), w.begin() + n)};
    }
    struct Tree {
        uint64_t parent = kNone;
        bool first = false;
        std::vector<uint64_t> children;
    };
    Tree tree(uint64_t kfId) {
        std::vector<int32_t> c(std::max<size_t>(kf_id_.size(), 1));
        int32_t p = -1, f = 0, n = 0;
        check("orbfe_map_get_spanning_tree",
              orbfe_map_get_spanning_tree(m_, kf(kfId), &p, &f, c.data(), (int)c.size(), &n));
        Tree t;
        if (p >= 0) t.parent = kf_id_[p];
        t.first = f != 0;
        c.resize((size_t)n);
        t.children = ids(c);
        return t;
    }
    orbfe_map* m_ = nullptr;
    std::vector<uint64_t> kf_id_, mp_id_;               // slot -> mnId
    std::unordered_map<uint64_t, int32_t> kf_slot_, mp_slot_;
    std::unordered_map<int32_t, std::vector<int32_t>> children_;
};

}  // namespace orbfe
