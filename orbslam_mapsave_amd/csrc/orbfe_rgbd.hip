// orbfe_rgbd.hip — MI355X (gfx950) replacement for the RGB-D frame path of
// skaegy/ORBSLAM_MapSave: what makes a Frame an RGB-D frame, and the consumers of mvDepth in
// tracking.
//
//   R1 rgbd_stereo_kernel    Frame::ComputeStereoFromRGBD (Frame.cc:759-780) with the depth
//                            conversion of Tracking::GrabImageRGBD (Tracking.cc:367-368) fused:
//                            one thread per keypoint reads the one raw pixel under it and scales
//                            it in registers; the converted plane is never made
//   R2 close_points_kernel   the close-point rule of Tracking::UpdateLastFrame (Tracking.cc:
//                            1059-1111) and CreateNewKeyFrame (1333-1392), StereoInitialization's
//                            take-all (764-779), the counters of NeedNewKeyFrame (1256-1265),
//                            Frame::UnprojectStereo (Frame.cc:782-796) and the distances of the
//                            Frame-form MapPoint constructor (MapPoint.cc:298-305); one workgroup
//                            per frame: ballot compaction of z > 0 in index order, an LDS bitonic
//                            sort of the distinct keys float_bits(z) << 32 | i, the visited prefix
//                            in closed form, then one thread per visit
//
// Every float expression follows the reference operation by operation (-ffp-contract=off); the
// conversion has one reading.
#include <hip/hip_runtime.h>

#include "../../include/orbfe.h"
#include "orbfe_device.hpp"
#include "orbfe_internal.hpp"

namespace orbfe {

// ---- R1 ------------------------------------------------------------------------------------
struct RgbdArgs {
    const uint8_t* depth;  // frame 0, raw plane
    long long fpitch;      // bytes between frames
    long long pitch;       // bytes between rows
    int type, w, h, kps_cap;
    float factor, bf;
    const orbfe_keypoint* keys;     // [frame][kps_cap] mvKeys
    const orbfe_keypoint* keys_un;  // [frame][kps_cap] mvKeysUn, or null: mvKeys
    const int* n;                   // [frame]
    float* u_right;                 // [frame][kps_cap]
    float* depth_out;               // [frame][kps_cap]
    int* status;  // ORBFE_ERR_UNSUPPORTED when a keypoint lies outside the depth image
};

constexpr int kRgbdBlock = 256;

__global__ __launch_bounds__(kRgbdBlock) void rgbd_stereo_kernel(RgbdArgs a) {
    const int f = blockIdx.y;
    const int i = blockIdx.x * kRgbdBlock + threadIdx.x;
    if (i >= min(a.n[f], a.kps_cap)) return;
    const size_t o = (size_t)f * a.kps_cap + i;
    const orbfe_keypoint kp = a.keys[o];
    // imDepth.at<float>(v, u): float -> int truncates toward zero, so -1 < u < 0 reads column 0;
    // the float comparisons hold exactly for w, h < 2^24 and fail for NaN
    float ur = -1.0f, dp = -1.0f;  // 761-762
    if (kp.x > -1.0f && kp.x < (float)a.w && kp.y > -1.0f && kp.y < (float)a.h) {
        const int col = (int)kp.x, row = (int)kp.y;
        const uint8_t* r = a.depth + f * a.fpitch + row * a.pitch;
        // convertTo(CV_32F, alpha): src * alpha (+ 0), exact in double for either source type
        const float d = a.type == ORBFE_DEPTH_U16
                            ? (float)reinterpret_cast<const uint16_t*>(r)[col] * a.factor
                            : reinterpret_cast<const float*>(r)[col] * a.factor;
        if (d > 0) {  // 774
            const float ux = a.keys_un ? a.keys_un[o].x : kp.x;
            dp = d;
            ur = ux - a.bf / d;
        }
    } else {
        atomicExch(a.status, ORBFE_ERR_UNSUPPORTED);
    }
    a.u_right[o] = ur;
    a.depth_out[o] = dp;
}

// ---- R2 ------------------------------------------------------------------------------------
constexpr int kCloseBlock = 1024;

struct CloseArgs {
    int mode, kps_cap, min_points, nlevels;
    int lds_keys;  // keys the dynamic LDS holds (a power of two, <= ORBFE_CLOSE_MAX_KEPT)
    const orbfe_keypoint* keys;  // [frame][kps_cap] mvKeysUn
    const float* depth;          // [frame][kps_cap] mvDepth
    const uint8_t* has_point;    // [frame][kps_cap], or null
    const int* n;                // [frame]
    const float* rwc_ow;         // [frame][12]
    float fx, fy, cx, cy, th;
    float scale[kMaxLevels];
    int* order;        // [frame][kps_cap]
    int* n_visited;    // [frame]
    uint8_t* create;   // [frame][kps_cap]
    float* xyz;        // [frame][kps_cap][3]
    float* max_dist;   // [frame][kps_cap], or null
    float* min_dist;
    int* n_total;      // [frame]
    int* n_map;
    int* status;       // [frame], zeroed before the launch
};

__global__ __launch_bounds__(kCloseBlock) void close_points_kernel(CloseArgs a) {
    extern __shared__ unsigned long long s_keys[];
    __shared__ int s_wave[kCloseBlock / 64];
    __shared__ int s_cnt[3];  // depths <= th among the kept, nTotal, nMap
    const int f = blockIdx.x;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int n = min(max(a.n[f], 0), a.kps_cap);
    const size_t fo = (size_t)f * a.kps_cap;
    const float* depth = a.depth + fo;
    const uint8_t* hp = a.has_point ? a.has_point + fo : nullptr;
    if (threadIdx.x < 3) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    // vDepthIdx (1063-1070): z > 0 kept in index order; NaN, +-0 and negatives drop out
    int kept = 0;
    for (int c0 = 0; c0 < n; c0 += kCloseBlock) {
        const int i = c0 + threadIdx.x;
        const float z = i < n ? depth[i] : 0.0f;
        const bool keep = z > 0;
        const bool near = keep && z < a.th;  // 1258
        const unsigned long long mk = __ballot(keep);
        const unsigned long long ml = __ballot(keep && !(z > a.th));
        const unsigned long long mt = __ballot(near);
        const unsigned long long mm = __ballot(near && hp && hp[i]);
        if (lane == 0) {
            s_wave[wid] = __popcll(mk);
            if (ml) atomicAdd(&s_cnt[0], __popcll(ml));
            if (mt) atomicAdd(&s_cnt[1], __popcll(mt));
            if (mm) atomicAdd(&s_cnt[2], __popcll(mm));
        }
        __syncthreads();
        int before = 0, total = 0;
        for (int w = 0; w < kCloseBlock / 64; ++w) {
            const int c = s_wave[w];
            before += w < wid ? c : 0;
            total += c;
        }
        if (keep) {
            const int pos = kept + before + __popcll(mk & ((1ull << lane) - 1));
            if (pos < a.lds_keys) s_keys[pos] = ((unsigned long long)__float_as_uint(z) << 32) | (unsigned)i;
        }
        kept += total;
        __syncthreads();
    }
    if (kept > ORBFE_CLOSE_MAX_KEPT) {  // nothing written
        if (threadIdx.x == 0) a.status[f] = ORBFE_ERR_CAPACITY;
        return;
    }
    int visited = kept;
    if (a.mode == ORBFE_CLOSE_SORTED) {
        // sort(vDepthIdx) (1075): positive floats and +inf order as their bit patterns and the
        // keys are distinct, so the order is the one std::sort of pair<float, int> gives
        int n_pad = 1;
        while (n_pad < kept) n_pad <<= 1;
        for (int t = kept + threadIdx.x; t < n_pad; t += kCloseBlock) s_keys[t] = ~0ull;
        __syncthreads();
        bitonic_sort_u64(s_keys, n_pad);
        // the walk (1080-1111): nPoints == j + 1 at the break test, which fires after the first
        // visit j with z_j > th and j >= min_points; z_j > th exactly for j >= c
        const long long stop = (long long)max(s_cnt[0], a.min_points) + 1;
        visited = (int)min((long long)kept, stop);
    }
    if (threadIdx.x == 0) {
        a.n_visited[f] = visited;
        a.n_total[f] = s_cnt[1];
        a.n_map[f] = s_cnt[2];
    }
    const orbfe_keypoint* keys = a.keys + fo;
    const float* R = a.rwc_ow + 12 * (size_t)f;
    const float invfx = 1.0f / a.fx, invfy = 1.0f / a.fy;  // Frame.cc:219-220
    for (int j = threadIdx.x; j < visited; j += kCloseBlock) {
        const unsigned long long key = s_keys[j];
        const int i = (int)(unsigned)key;
        const bool create = a.mode == ORBFE_CLOSE_ALL || !(hp && hp[i]);
        a.order[fo + j] = i;
        a.create[fo + j] = create ? 1 : 0;
        float P[3] = {0.0f, 0.0f, 0.0f}, dmax = 0.0f, dmin = 0.0f;
        if (create) {
            // UnprojectStereo (Frame.cc:784-792)
            const orbfe_keypoint k = keys[i];
            const float z = __uint_as_float((unsigned)(key >> 32));
            const float x = (k.x - a.cx) * z * invfx;
            const float y = (k.y - a.cy) * z * invfy;
#pragma unroll
            for (int r = 0; r < 3; ++r) P[r] = ((R[3 * r] * x + R[3 * r + 1] * y) + R[3 * r + 2] * z) + R[9 + r];
            if (a.max_dist) {
                // MapPoint.cc:298-305: cv::norm of a float vector accumulates in double
                const float d0 = P[0] - R[9], d1 = P[1] - R[10], d2 = P[2] - R[11];
                const float dist = (float)sqrt((double)d0 * d0 + (double)d1 * d1 + (double)d2 * d2);
                if (k.octave < 0 || k.octave >= a.nlevels) {
                    atomicExch(&a.status[f], ORBFE_ERR_UNSUPPORTED);  // mvScaleFactors[level]
                    dmax = dmin = -1.0f;
                } else {
                    dmax = dist * a.scale[k.octave];
                    dmin = dmax / a.scale[a.nlevels - 1];
                }
            }
        }
        a.xyz[3 * (fo + j)] = P[0];
        a.xyz[3 * (fo + j) + 1] = P[1];
        a.xyz[3 * (fo + j) + 2] = P[2];
        if (a.max_dist) {
            a.max_dist[fo + j] = dmax;
            a.min_dist[fo + j] = dmin;
        }
    }
}

}  // namespace orbfe

using namespace orbfe;

namespace {
size_t depth_elem(int depth_type) {
    return depth_type == ORBFE_DEPTH_U16 ? 2 : depth_type == ORBFE_DEPTH_F32 ? 4 : 0;
}

int launch_rgbd_stereo(orbfe_extractor* h, const RgbdArgs& a, int n_frames) {
    ORBFE_HIP(hipMemsetAsync(a.status, 0, sizeof(int), h->stream));
    hipLaunchKernelGGL(rgbd_stereo_kernel, dim3((a.kps_cap + kRgbdBlock - 1) / kRgbdBlock, n_frames),
                       dim3(kRgbdBlock), 0, h->stream, a);
    ORBFE_HIP(hipGetLastError());
    return ORBFE_OK;
}

int launch_close_points(orbfe_matcher* m, CloseArgs& a, int n_frames) {
    int keys = 64;
    while (keys < a.kps_cap && keys < ORBFE_CLOSE_MAX_KEPT) keys <<= 1;
    a.lds_keys = keys;
    const size_t lds = (size_t)keys * sizeof(unsigned long long);
    if (lds > 32 * 1024)  // with the kernel's static words the full sort passes 64 KB
        ORBFE_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&close_points_kernel),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    ORBFE_HIP(hipMemsetAsync(a.status, 0, (size_t)n_frames * sizeof(int), m->stream));
    hipLaunchKernelGGL(close_points_kernel, dim3(n_frames), dim3(kCloseBlock), lds, m->stream, a);
    ORBFE_HIP(hipGetLastError());
    return ORBFE_OK;
}

bool close_args_ok(int mode, const orbfe_camera* cam, const float* scale_factors, int nlevels,
                   bool dists) {
    if ((mode != ORBFE_CLOSE_SORTED && mode != ORBFE_CLOSE_ALL) || !cam) return false;
    return !dists || (scale_factors && nlevels >= 1 && nlevels <= kMaxLevels);
}

void close_fill(CloseArgs& a, int mode, int kps_cap, const orbfe_camera* cam, float th_depth,
                int min_points, const float* scale_factors, int nlevels, bool dists) {
    a.mode = mode;
    a.kps_cap = kps_cap;
    a.min_points = min_points;
    a.nlevels = dists ? nlevels : 0;
    a.fx = cam->fx;
    a.fy = cam->fy;
    a.cx = cam->cx;
    a.cy = cam->cy;
    a.th = th_depth;
    for (int l = 0; l < a.nlevels; ++l) a.scale[l] = scale_factors[l];
}
}  // namespace

extern "C" {

int orbfe_depth_buffer(orbfe_extractor* h, int w, int hgt, int depth_type, void** buf,
                       size_t* stride) {
    const size_t es = depth_elem(depth_type);
    if (!h || w <= 0 || hgt <= 0 || !es || !buf || !stride) return ORBFE_ERR_ARG;
    return guarded(h, [&]() {
        int st;
        if ((st = h->pin_depth.ensure((size_t)w * es * hgt))) return st;
        *buf = h->pin_depth.p;
        *stride = (size_t)w * es;
        return ORBFE_OK;
    });
}

int orbfe_compute_stereo_from_rgbd(orbfe_extractor* h, const void* depth, int depth_type, int w,
                                   int hgt, size_t stride, float depth_factor,
                                   const orbfe_keypoint* keys, const orbfe_keypoint* keys_un,
                                   int n, float bf, float* u_right, float* depth_out) {
    const size_t es = depth_elem(depth_type);
    if (!h || !depth || !es || w <= 0 || hgt <= 0 || stride < (size_t)w * es || stride % es ||
        n < 0 || (n && (!keys || !u_right || !depth_out)))
        return ORBFE_ERR_ARG;
    if (n == 0) return ORBFE_OK;
    return guarded(h, [&]() {
        int st;
        hipStream_t s = h->stream;
        auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
        const size_t kb = (size_t)n * sizeof(orbfe_keypoint), row = (size_t)w * es;
        const bool staged = depth == h->pin_depth.p && h->pin_depth.bytes >= stride * (hgt - 1) + row;
        // keys | keys_un | count, then (a foreign plane) its rows packed; outputs u_right | depth |
        // status come back into the same pinned block
        const size_t o_un = al(kb), o_n = o_un + (keys_un ? al(kb) : 0), o_img = o_n + 256,
                     in_bytes = o_img + (staged ? 0 : al(row * hgt)), o_dp = al((size_t)n * 4),
                     o_st = 2 * o_dp, out_bytes = o_st + 256;
        if ((st = h->rg_pin.ensure(std::max(in_bytes, out_bytes)))) return st;
        if ((st = h->rg_in.ensure(in_bytes))) return st;
        if ((st = h->rg_out.ensure(out_bytes))) return st;
        if ((st = h->rg_status.ensure(sizeof(int)))) return st;
        uint8_t* q = h->rg_pin.p;
        std::memcpy(q, keys, kb);
        if (keys_un) std::memcpy(q + o_un, keys_un, kb);
        const int32_t cnt = n;
        std::memcpy(q + o_n, &cnt, sizeof(cnt));
        uint8_t* din = h->rg_in.as<uint8_t>();
        RgbdArgs a{};
        if (!staged) {
            for (int y = 0; y < hgt; ++y)
                std::memcpy(q + o_img + y * row, static_cast<const uint8_t*>(depth) + y * stride, row);
            a.depth = din + o_img;
            a.pitch = (long long)row;
        } else if (h->sw.zero_copy && h->pin_depth.d) {
            a.depth = h->pin_depth.d;  // gathered in place: about n cache lines cross the link
            a.pitch = (long long)stride;
        } else {
            if ((st = h->rg_depth.ensure(stride * hgt))) return st;
            ORBFE_HIP(hipMemcpyAsync(h->rg_depth.p, depth, stride * (hgt - 1) + row, hipMemcpyHostToDevice, s));
            a.depth = h->rg_depth.as<uint8_t>();
            a.pitch = (long long)stride;
        }
        ORBFE_HIP(hipMemcpyAsync(din, q, in_bytes, hipMemcpyHostToDevice, s));
        uint8_t* dout = h->rg_out.as<uint8_t>();
        a.fpitch = 0;
        a.type = depth_type;
        a.w = w;
        a.h = hgt;
        a.kps_cap = n;
        a.factor = depth_factor;
        a.bf = bf;
        a.keys = reinterpret_cast<const orbfe_keypoint*>(din);
        a.keys_un = keys_un ? reinterpret_cast<const orbfe_keypoint*>(din + o_un) : nullptr;
        a.n = reinterpret_cast<const int*>(din + o_n);
        a.u_right = reinterpret_cast<float*>(dout);
        a.depth_out = reinterpret_cast<float*>(dout + o_dp);
        a.status = h->rg_status.as<int>();
        if ((st = launch_rgbd_stereo(h, a, 1))) return st;
        ORBFE_HIP(hipMemcpyAsync(dout + o_st, a.status, sizeof(int), hipMemcpyDeviceToDevice, s));
        ORBFE_HIP(hipMemcpyAsync(q, dout, out_bytes, hipMemcpyDeviceToHost, s));
        ORBFE_HIP(hipStreamSynchronize(s));
        std::memcpy(u_right, q, (size_t)n * sizeof(float));
        std::memcpy(depth_out, q + o_dp, (size_t)n * sizeof(float));
        int status = 0;
        std::memcpy(&status, q + o_st, sizeof(int));
        return status;
    });
}

int orbfe_compute_stereo_from_rgbd_device(orbfe_extractor* h, int n_frames, const void* d_depth,
                                          int depth_type, int w, int hgt, size_t stride,
                                          size_t frame_pitch, float depth_factor,
                                          const orbfe_keypoint* d_keys,
                                          const orbfe_keypoint* d_keys_un, const int32_t* d_n,
                                          int kps_cap, float bf, float* d_u_right,
                                          float* d_depth_out) {
    const size_t es = depth_elem(depth_type);
    if (!h || n_frames < 0 || !d_depth || !es || w <= 0 || hgt <= 0 || stride < (size_t)w * es ||
        stride % es || (uintptr_t)d_depth % es || frame_pitch % es ||
        (n_frames > 1 && frame_pitch < stride * hgt) || !d_keys || !d_n || kps_cap <= 0 ||
        !d_u_right || !d_depth_out)
        return ORBFE_ERR_ARG;
    if (n_frames == 0) return ORBFE_OK;
    return guarded(h, [&]() {
        int st;
        if ((st = h->rg_status.ensure(sizeof(int)))) return st;
        RgbdArgs a{};
        a.depth = static_cast<const uint8_t*>(d_depth);
        a.fpitch = (long long)frame_pitch;
        a.pitch = (long long)stride;
        a.type = depth_type;
        a.w = w;
        a.h = hgt;
        a.kps_cap = kps_cap;
        a.factor = depth_factor;
        a.bf = bf;
        a.keys = d_keys;
        a.keys_un = d_keys_un;
        a.n = d_n;
        a.u_right = d_u_right;
        a.depth_out = d_depth_out;
        a.status = h->rg_status.as<int>();
        return launch_rgbd_stereo(h, a, n_frames);
    });
}

int orbfe_rgbd_status(orbfe_extractor* h) {
    if (!h) return ORBFE_ERR_ARG;
    if (!h->rg_status.p) return ORBFE_OK;
    DeviceGuard dg(h->device);
    int status = 0;
    ORBFE_HIP(hipMemcpyAsync(&status, h->rg_status.p, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    ORBFE_HIP(hipStreamSynchronize(h->stream));
    return status;
}

int orbfe_close_points(orbfe_matcher* m, int mode, const orbfe_keypoint* keys_un,
                       const float* depth, const uint8_t* has_point, int n,
                       const orbfe_camera* cam, const float* rwc_ow, float th_depth,
                       int min_points, const float* scale_factors, int nlevels, int32_t* order,
                       int32_t* n_visited, uint8_t* create, float* xyz, float* max_dist,
                       float* min_dist, int32_t* n_total, int32_t* n_map) {
    const bool dists = max_dist || min_dist;
    if (!m || n < 0 || !close_args_ok(mode, cam, scale_factors, nlevels, dists) || !rwc_ow ||
        !n_visited || !n_total || !n_map || (dists && (!max_dist || !min_dist)) ||
        (n && (!keys_un || !depth || !order || !create || !xyz ||
               (mode == ORBFE_CLOSE_SORTED && !has_point))))
        return ORBFE_ERR_ARG;
    if (n == 0) {
        *n_visited = *n_total = *n_map = 0;
        return ORBFE_OK;
    }
    return guarded(m, [&]() {
        int st;
        const int32_t head[5] = {0, 0, 0, 0, n};  // n_visited, n_total, n_map, status | count
        if ((st = m->up(m->fa_k, keys_un, (size_t)n * sizeof(orbfe_keypoint)))) return st;
        if ((st = m->up(m->m_f0, depth, (size_t)n * 4))) return st;
        if (has_point && (st = m->up(m->m_u0, has_point, n))) return st;
        if ((st = m->up(m->m_f1, rwc_ow, 12 * sizeof(float)))) return st;
        if ((st = m->up(m->scal, head, sizeof(head)))) return st;
        if ((st = m->o_i.ensure((size_t)n * 4))) return st;
        if ((st = m->o_u.ensure(n))) return st;
        if ((st = m->o_f0.ensure((size_t)n * 12))) return st;
        if ((st = m->o_f1.ensure((size_t)n * 4))) return st;
        if ((st = m->o_f2.ensure((size_t)n * 4))) return st;
        if ((st = m->flush())) return st;
        CloseArgs a{};
        close_fill(a, mode, n, cam, th_depth, min_points, scale_factors, nlevels, dists);
        a.keys = m->fa_k.as<orbfe_keypoint>();
        a.depth = m->m_f0.as<float>();
        a.has_point = has_point ? m->m_u0.as<uint8_t>() : nullptr;
        a.rwc_ow = m->m_f1.as<float>();
        int* sc = m->scal.as<int>();
        a.n = sc + 4;
        a.order = m->o_i.as<int>();
        a.n_visited = sc;
        a.create = m->o_u.as<uint8_t>();
        a.xyz = m->o_f0.as<float>();
        a.max_dist = dists ? m->o_f1.as<float>() : nullptr;
        a.min_dist = dists ? m->o_f2.as<float>() : nullptr;
        a.n_total = sc + 1;
        a.n_map = sc + 2;
        a.status = sc + 3;
        if ((st = launch_close_points(m, a, 1))) return st;
        // the prefix the caller receives is known only with the counters: everything comes down
        // into the staging block and the visited part goes on from there
        const int32_t* res;
        const int32_t* q_order;
        const uint8_t* q_create;
        const float *q_xyz, *q_max = nullptr, *q_min = nullptr;
        if ((st = m->stg.down_staged(sc, 4 * sizeof(int32_t), &res))) return st;
        if ((st = m->stg.down_staged(a.order, (size_t)n * 4, &q_order))) return st;
        if ((st = m->stg.down_staged(a.create, (size_t)n, &q_create))) return st;
        if ((st = m->stg.down_staged(a.xyz, (size_t)n * 12, &q_xyz))) return st;
        if (dists) {
            if ((st = m->stg.down_staged(a.max_dist, (size_t)n * 4, &q_max))) return st;
            if ((st = m->stg.down_staged(a.min_dist, (size_t)n * 4, &q_min))) return st;
        }
        if ((st = m->sync())) return st;
        if (res[3] == ORBFE_ERR_CAPACITY) return ORBFE_ERR_CAPACITY;
        const size_t v = (size_t)res[0];
        std::memcpy(order, q_order, v * 4);
        std::memcpy(create, q_create, v);
        std::memcpy(xyz, q_xyz, v * 12);
        if (dists) {
            std::memcpy(max_dist, q_max, v * 4);
            std::memcpy(min_dist, q_min, v * 4);
        }
        *n_visited = res[0];
        *n_total = res[1];
        *n_map = res[2];
        return res[3];
    });
}

int orbfe_close_points_batch_device(orbfe_matcher* m, int mode, int n_frames,
                                    const orbfe_keypoint* d_keys_un, const float* d_depth,
                                    const uint8_t* d_has_point, const int32_t* d_n, int kps_cap,
                                    const orbfe_camera* cam, const float* d_rwc_ow,
                                    float th_depth, int min_points, const float* scale_factors,
                                    int nlevels, int32_t* d_order, int32_t* d_n_visited,
                                    uint8_t* d_create, float* d_xyz, float* d_max_dist,
                                    float* d_min_dist, int32_t* d_n_total, int32_t* d_n_map,
                                    int32_t* d_status) {
    const bool dists = d_max_dist || d_min_dist;
    if (!m || n_frames < 0 || kps_cap <= 0 ||
        !close_args_ok(mode, cam, scale_factors, nlevels, dists) || !d_keys_un || !d_depth ||
        (mode == ORBFE_CLOSE_SORTED && !d_has_point) || !d_n || !d_rwc_ow || !d_order ||
        !d_n_visited || !d_create || !d_xyz || (dists && (!d_max_dist || !d_min_dist)) ||
        !d_n_total || !d_n_map || !d_status)
        return ORBFE_ERR_ARG;
    if (n_frames == 0) return ORBFE_OK;
    return guarded(m, [&]() {
        CloseArgs a{};
        close_fill(a, mode, kps_cap, cam, th_depth, min_points, scale_factors, nlevels, dists);
        a.keys = d_keys_un;
        a.depth = d_depth;
        a.has_point = d_has_point;
        a.n = d_n;
        a.rwc_ow = d_rwc_ow;
        a.order = d_order;
        a.n_visited = d_n_visited;
        a.create = d_create;
        a.xyz = d_xyz;
        a.max_dist = d_max_dist;
        a.min_dist = d_min_dist;
        a.n_total = d_n_total;
        a.n_map = d_n_map;
        a.status = d_status;
        return launch_close_points(m, a, n_frames);
    });
}

}  // extern "C"
