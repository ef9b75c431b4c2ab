// orbfe_refresh.hip — MapPoint::UpdateNormalAndDepth (MapPoint.cc:571-619) and
// ComputeDistinctiveDescriptors (:483-548) on an orbfe_map, the map-point loop of
// LocalMapping::ProcessNewKeyFrame (LocalMapping.cc:140-161), and the state the two functions read
// that the map did not hold yet: mvScaleFactors per map; GetCameraCenter() and
// whether the descriptors were set per keyframe; the descriptor row per keyframe keypoint, in a
// side pool of kf_mp; mpRefKF per point.  The columns, the pool and their growth are the store's
// (orbfe_map_store.hip); the erases that keep mpRefKF are where the erases are (orbfe_cull.hip,
// orbfe_localmap.hip).
//
//   refresh_kernel    one wave per listed point, lanes over its observers.  Launched twice:
//                     checking (writes nothing but the call's error word) and applying (nothing
//                     if that word holds a refusal).  The row, stored by keyframe slot, is sorted
//                     by order key first ("pointer order", H26): at N <= 64 by counting ranks over
//                     shuffles, above that bitonic in LDS (1,024 x 8 bytes per wave).  The normal:
//                     the lanes compute Pos - Ow_i and the float reciprocal of its double norm,
//                     one lane adds the terms in key order.  The descriptor: observers of bad
//                     keyframes leave the sorted row, up to 64 descriptors are staged in LDS, the
//                     median and winner rule is distinctive_best (orbfe_match.hip).  The last
//                     workgroup of the applying launch reports through the pinned block.
//   refresh_classify_kernel   one thread per slot of a keyframe: NULL or bad, not yet observed by
//                     the keyframe, or observed already (LocalMapping.cc:145-149)
//
// Everything but the normal is integer-exact or a single IEEE operation; the normal's readings of
// cv::Mat arithmetic are one helper each (refresh_recip, refresh_axpy, refresh_mean).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <unordered_set>
#include <vector>

#include "../../include/orbfe.h"
#include "orbfe_device.hpp"

namespace orbfe {

constexpr int kRefBlock = 256;
constexpr int kRefWaves = kRefBlock / 64;
constexpr int kRefMaxObs = ORBFE_MAP_MAX_REFRESH_OBS;
constexpr int kRefChunks = kRefMaxObs / 64;
enum { kRefErrArg = 1, kRefErrCapacity = 2, kRefErrUnsupported = 4 };  // bits of the call's error word

struct MapVec3 {
    float v[3];
};

struct RefreshDev {
    const int* ref_kf;         // [n_mp]
    const float* center;       // [3 n_kf]
    const uint8_t* desc_set;   // [n_kf]
    const uint4* kdesc;        // two per keypoint, at the offsets of kf_mp's pool
    const uint8_t* feat;       // octave | kCullRight, at the same offsets
    const float* scale;        // [nlevels]
    int nlevels;
};

struct RefreshArgs {
    MapDev d;
    RefreshDev r;
    int what, n, apply;
    int extra;                 // checking only: observers each listed point is about to gain
    const int* list;           // [n] point slots or -1
    orbfe_map_point_arrays arr;
    uint8_t* result;           // [n] or NULL
    int* res;                  // the handle's pinned block
};

// cv::norm of a 3x1 CV_32F: the squares summed in double, in index order (H25).
__device__ __forceinline__ double refresh_norm(float d0, float d1, float d2) {
    return sqrt(((double)d0 * d0 + (double)d1 * d1) + (double)d2 * d2);
}
// The three readings of cv::Mat arithmetic (H29).  Mat / double: the scale 1 / s taken as a float.
__device__ __forceinline__ float refresh_recip(double s) { return (float)(1.0 / s); }
// Mat + Mat * a: the product rounded, then the sum.
__device__ __forceinline__ float refresh_axpy(float acc, float d, float a) {
    const float t = d * a;
    return acc + t;
}
// Mat / int: the scale 1 / n taken as a float.
__device__ __forceinline__ float refresh_mean(float acc, int n) { return acc * refresh_recip((double)n); }

// LDS writes of this wave ahead of LDS reads of this wave.
__device__ __forceinline__ void refresh_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ unsigned long long refresh_pack(int kf, int ix) {
    return (unsigned long long)(unsigned)kf | ((unsigned long long)(unsigned)ix << 32);
}

// The observers of a point as (keyframe, index) in ascending order key, into row[0 .. N).
__device__ __forceinline__ void refresh_sort_row(const MapDev& d, long long oo, int N, int lane,
                                                 unsigned long long* row) {
    const auto key_at = [&](int j) {
        const int kf = d.mp_obs[oo + j];
        return kf >= 0 && kf < d.n_kf ? d.kf_key[kf] : ~0ull;
    };
    if (N <= 64) {
        const bool in = lane < N;
        const unsigned long long key = in ? key_at(lane) : ~0ull;
        int rank = 0;
        for (int t = 0; t < N; ++t) {  // keys are distinct; the lane breaks a tie all the same
            const unsigned long long kt = __shfl(key, t, 64);
            rank += kt < key || (kt == key && t < lane);
        }
        if (in) row[rank] = refresh_pack(d.mp_obs[oo + lane], d.mp_idx[oo + lane]);
        refresh_wave_sync();
        return;
    }
    int P = 128;
    while (P < N) P <<= 1;
    for (int t = lane; t < P; t += 64) row[t] = t < N ? key_at(t) : ~0ull;
    refresh_wave_sync();
    for (int size = 2; size <= P; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = lane; t < P / 2; t += 64) {
                const int lo = 2 * t - (t & (stride - 1));
                const int hi = lo + stride;
                const bool up = (lo & size) == 0;
                const unsigned long long x = row[lo], y = row[hi];
                if ((x > y) == up) {
                    row[lo] = y;
                    row[hi] = x;
                }
            }
            refresh_wave_sync();
        }
    int rank[kRefChunks];
#pragma unroll
    for (int c = 0; c < kRefChunks; ++c) {
        const int j = c * 64 + lane;
        rank[c] = 0;
        if (j < N) {
            const unsigned long long key = key_at(j);
            int lo = 0, hi = N;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (row[mid] < key) lo = mid + 1;
                else hi = mid;
            }
            rank[c] = min(lo, N - 1);
        }
    }
    refresh_wave_sync();
#pragma unroll
    for (int c = 0; c < kRefChunks; ++c) {
        const int j = c * 64 + lane;
        if (j < N) row[rank[c]] = refresh_pack(d.mp_obs[oo + j], d.mp_idx[oo + j]);
    }
    refresh_wave_sync();
}

// One listed point, by one whole wave.  -1: the entry is skipped (NULL, bad, refused); otherwise
// the mask of what was written, the same in every lane.
__device__ __forceinline__ int refresh_point(const RefreshArgs& a, int i, int lane, unsigned long long* row,
                                             uint4* stage, float* term) {
    const MapDev& d = a.d;
    const RefreshDev& r = a.r;
    int* const err = &d.ctl[kCtlCallErr];
    const int mp = a.list[i];
    if (mp == -1) return -1;
    if (mp < -1 || mp >= d.n_mp) {
        if (!a.apply && lane == 0) atomicOr(err, kRefErrArg);
        return -1;
    }
    if (d.mp_bad[mp]) return -1;  // mbBad returns first in both functions (:492, :579)
    const long long oo = d.mp_obs_off[mp];
    const int N = d.mp_obs_n[mp];
    if (N + a.extra > kRefMaxObs) {
        if (!a.apply && lane == 0) atomicOr(err, kRefErrCapacity);
        return -1;
    }
    if (N <= 0) return 0;  // observations.empty() (:497, :586)
    // pRefKF, `observations[pRefKF]` (operator[]: index 0 when it is not an observer) and the level
    const int ref = (a.what & ORBFE_MAP_REFRESH_NORMAL_DEPTH) ? r.ref_kf[mp] : -1;
    bool unsupported = false;
    int level = 0;
    if (ref >= 0 && ref < d.n_kf) {
        int p = -1;
        for (int c = 0; c < N && p < 0; c += 64) {
            const int j = c + lane;
            const unsigned long long b = __ballot(j < N && d.mp_obs[oo + j] == ref);
            if (b) p = c + __ffsll((long long)b) - 1;
        }
        const int ix = p >= 0 ? d.mp_idx[oo + p] : 0;
        if (ix < 0 || ix >= d.kf_mp_n[ref]) unsupported = true;  // no keypoint to read
        else {
            level = r.feat[d.kf_mp_off[ref] + ix] & (kCullRight - 1);
            if (level >= r.nlevels) unsupported = true;
        }
    }
    if (!a.apply) {
        bool refuse = false;
        for (int j = lane; j < N; j += 64) {
            const int kf = d.mp_obs[oo + j], ix = d.mp_idx[oo + j];
            if (kf < 0 || kf >= d.n_kf || ix < 0 || ix >= d.kf_mp_n[kf]) refuse = true;
            else if ((a.what & ORBFE_MAP_REFRESH_DESCRIPTOR) && !d.kf_bad[kf] && !r.desc_set[kf]) refuse = true;
        }
        if (__ballot(refuse)) {
            if (lane == 0) atomicOr(err, kRefErrArg);
        } else if (unsupported && lane == 0) {
            atomicOr(err, kRefErrUnsupported);
        }
        return -1;
    }
    refresh_sort_row(d, oo, N, lane, row);
    int mask = 0;
    if (ref >= 0 && ref < d.n_kf && unsupported) mask |= ORBFE_MAP_REFRESH_UNSUPPORTED;
    if (ref >= 0 && ref < d.n_kf && !unsupported) {  // pRefKF == NULL: all three stay (:600)
        const float P0 = a.arr.xyz[3 * (size_t)mp], P1 = a.arr.xyz[3 * (size_t)mp + 1],
                    P2 = a.arr.xyz[3 * (size_t)mp + 2];
        float acc0 = 0.f, acc1 = 0.f, acc2 = 0.f;
        for (int c = 0; c < N; c += 64) {  // every observer counts, bad keyframes too (:591-598)
            const int j = c + lane;
            if (j < N) {
                const int kf = (int)(unsigned)row[j];
                const float* ow = r.center + 3 * (size_t)kf;
                const float d0 = P0 - ow[0], d1 = P1 - ow[1], d2 = P2 - ow[2];
                term[4 * lane] = d0;
                term[4 * lane + 1] = d1;
                term[4 * lane + 2] = d2;
                term[4 * lane + 3] = refresh_recip(refresh_norm(d0, d1, d2));
            }
            refresh_wave_sync();
            if (lane == 0) {
                const int m = min(64, N - c);
                for (int t = 0; t < m; ++t) {  // sequential, in pointer order
                    const float s = term[4 * t + 3];
                    acc0 = refresh_axpy(acc0, term[4 * t], s);
                    acc1 = refresh_axpy(acc1, term[4 * t + 1], s);
                    acc2 = refresh_axpy(acc2, term[4 * t + 2], s);
                }
            }
            refresh_wave_sync();
        }
        if (lane == 0) {
            const float* ow = r.center + 3 * (size_t)ref;  // no isBad test on pRefKF
            const float dist = (float)refresh_norm(P0 - ow[0], P1 - ow[1], P2 - ow[2]);
            const float maxd = dist * r.scale[level];
            a.arr.max_dist[mp] = maxd;
            a.arr.min_dist[mp] = maxd / r.scale[r.nlevels - 1];
            a.arr.normal[3 * (size_t)mp] = refresh_mean(acc0, N);
            a.arr.normal[3 * (size_t)mp + 1] = refresh_mean(acc1, N);
            a.arr.normal[3 * (size_t)mp + 2] = refresh_mean(acc2, N);
        }
        mask |= ORBFE_MAP_REFRESH_NORMAL_DEPTH;
    }
    if (a.what & ORBFE_MAP_REFRESH_DESCRIPTOR) {
        // the observers whose keyframe is not bad (:506), in order, as elements of the pool; the
        // row closes up in place: every lane loads before any lane stores, at or below its place
        int M = 0;
        for (int c = 0; c < N; c += 64) {
            const int j = c + lane;
            bool keep = false;
            unsigned long long e = 0;
            if (j < N) {
                const int kf = (int)(unsigned)row[j], ix = (int)(row[j] >> 32);
                keep = !d.kf_bad[kf];
                e = (unsigned long long)(d.kf_mp_off[kf] + ix);
            }
            const unsigned long long b = __ballot(keep);
            refresh_wave_sync();
            if (keep) row[M + __popcll(b & ((1ull << lane) - 1))] = e;
            M += __popcll(b);
            refresh_wave_sync();
        }
        if (M > 0) {  // vDescriptors.empty(): mDescriptor stays (:510)
            int best;
            if (M <= kDdStage) {
                for (int k = lane; k < 2 * M; k += 64) stage[k] = r.kdesc[2 * row[k >> 1] + (k & 1)];
                refresh_wave_sync();
                best = distinctive_best(M, lane, [stage](int j, uint4& d0, uint4& d1) {
                    d0 = stage[2 * j];
                    d1 = stage[2 * j + 1];
                });
            } else {
                const uint4* kdesc = r.kdesc;
                best = distinctive_best(M, lane, [kdesc, row](int j, uint4& d0, uint4& d1) {
                    const uint4* p = kdesc + 2 * row[j];
                    d0 = p[0];
                    d1 = p[1];
                });
            }
            if (lane < 2)
                reinterpret_cast<uint4*>(a.arr.desc)[2 * (size_t)mp + lane] = r.kdesc[2 * row[best] + lane];
            mask |= ORBFE_MAP_REFRESH_DESCRIPTOR;
        }
    }
    return mask;
}

__global__ __launch_bounds__(kRefBlock) void refresh_kernel(RefreshArgs a) {
    __shared__ unsigned long long s_row[kRefWaves][kRefMaxObs];
    __shared__ uint4 s_stage[kRefWaves][2 * kDdStage];
    __shared__ float s_term[kRefWaves][4 * 64];
    const MapDev& d = a.d;
    const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int i = blockIdx.x * kRefWaves + wid;
    const bool refused = a.apply && (d.ctl[kCtlCallErr] & (kRefErrArg | kRefErrCapacity));
    if (i < a.n && !refused) {
        const int mask = refresh_point(a, i, lane, s_row[wid], s_stage[wid], s_term[wid]);
        if (a.apply && lane == 0) {
            if (a.result) a.result[i] = (uint8_t)max(mask, 0);
            if (mask >= 0) atomicAdd(&d.ctl[kCtlCountB], 1);
            __threadfence_system();
        }
    }
    if (!a.apply) return;
    if (!map_last_workgroup(&d.ctl[kCtlCountA], gridDim.x)) return;
    if (threadIdx.x == 0) {
        a.res[kResStatus] = d.ctl[kCtlCallErr];
        a.res[kResValue] = __hip_atomic_load(&d.ctl[kCtlCountB], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        d.ctl[kCtlCountA] = 0;
        d.ctl[kCtlCountB] = 0;
        __threadfence_system();
        __hip_atomic_store(&a.res[kResDone], 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// LocalMapping.cc:145-149 for every slot of keyframe kf: out[2 i] = the point, out[2 i + 1] = 0 (NULL
// or bad), 1 (the keyframe is not among its observers) or 2 (it is).
__global__ __launch_bounds__(kRefBlock) void refresh_classify_kernel(MapDev d, int kf, int* out, int* res) {
    const int i = blockIdx.x * kRefBlock + threadIdx.x;
    if (i < d.kf_mp_n[kf]) {
        const int mp = d.kf_mp[d.kf_mp_off[kf] + i];
        int cls = 0;
        if (mp >= 0 && mp < d.n_mp && !d.mp_bad[mp]) {
            cls = 1;
            const long long oo = d.mp_obs_off[mp];
            const int no = d.mp_obs_n[mp];
            for (int j = 0; j < no; ++j)
                if (d.mp_obs[oo + j] == kf) cls = 2;
        }
        out[2 * i] = mp;
        out[2 * i + 1] = cls;
        __threadfence_system();
    }
    if (!map_last_workgroup(&d.ctl[kCtlCountA], gridDim.x)) return;
    if (threadIdx.x == 0) {
        d.ctl[kCtlCountA] = 0;
        __threadfence_system();
        __hip_atomic_store(&res[kResDone], 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

}  // namespace orbfe

namespace {

RefreshDev refresh_dev(const orbfe_map* m) {
    RefreshDev r;
    r.ref_kf = m->at<int>(kColRefKf);
    r.center = m->at<float>(kColCenter);
    r.desc_set = m->at<uint8_t>(kColDescSet);
    r.kdesc = m->kdesc_pool.buf.as<uint4>();
    r.feat = m->feat_pool.buf.as<uint8_t>();
    r.scale = m->scale.as<float>();
    r.nlevels = (int)m->h_scale.size();
    return r;
}

bool refresh_args_ok(const orbfe_map* m, int what, int n, const void* list,
                     const orbfe_map_point_arrays* a) {
    if (!m || n < 0 || (n && !list) || !a) return false;
    if (what < 1 || what > (ORBFE_MAP_REFRESH_NORMAL_DEPTH | ORBFE_MAP_REFRESH_DESCRIPTOR)) return false;
    if ((what & ORBFE_MAP_REFRESH_NORMAL_DEPTH) &&
        (!a->xyz || !a->normal || !a->min_dist || !a->max_dist || m->h_scale.empty()))
        return false;
    if ((what & ORBFE_MAP_REFRESH_DESCRIPTOR) && (!a->desc || ((uintptr_t)a->desc & 15))) return false;
    return true;
}

// Both launches over the device list; waits on the done word.  ORBFE_ERR_UNSUPPORTED comes back
// with everything else written.
int refresh_run(orbfe_map* m, int what, int n, const int* d_list, const orbfe_map_point_arrays& arr,
                uint8_t* d_result, int* n_live, int check_extra = -1) {
    int st;
    if ((st = cull_ready(m))) return st;
    if ((st = store_side_pools(m))) return st;  // the octaves
    if ((st = ref_ready_mp(m))) return st;
    if ((st = ref_ready_kf(m))) return st;
    if ((what & ORBFE_MAP_REFRESH_DESCRIPTOR) && (st = store_desc_pool(m))) return st;
    if ((st = store_clear_err(m))) return st;
    int* res = m->pin;
    res[kResStatus] = 0;
    res[kResValue] = 0;
    __atomic_store_n(&res[kResDone], -1, __ATOMIC_RELEASE);
    RefreshArgs a{};
    a.d = m->dev();
    a.r = refresh_dev(m);
    a.what = what;
    a.n = n;
    a.list = d_list;
    a.arr = arr;
    a.result = d_result;
    a.res = m->pin_dev;
    const dim3 grid((unsigned)((n + kRefWaves - 1) / kRefWaves));
    if (check_extra >= 0) {  // the check launch alone, for points about to gain observers
        a.extra = check_extra;
        int err = 0;
        hipLaunchKernelGGL(refresh_kernel, grid, dim3(kRefBlock), 0, m->stream, a);
        ORBFE_HIP(hipGetLastError());
        if ((st = store_read_err(m, err))) return st;
        return err & kRefErrArg ? ORBFE_ERR_ARG : err & kRefErrCapacity ? ORBFE_ERR_CAPACITY : ORBFE_OK;
    }
    for (a.apply = 0; a.apply < 2; ++a.apply)
        hipLaunchKernelGGL(refresh_kernel, grid, dim3(kRefBlock), 0, m->stream, a);
    ORBFE_HIP(hipGetLastError());
    if ((st = wait_words(res + kResDone, 1, -1, m->stream, 20000))) return st;
    const int err = res[kResStatus];
    if (err & kRefErrArg) return ORBFE_ERR_ARG;
    if (err & kRefErrCapacity) return ORBFE_ERR_CAPACITY;
    if (n_live) *n_live = res[kResValue];
    return err & kRefErrUnsupported ? ORBFE_ERR_UNSUPPORTED : ORBFE_OK;
}

bool refresh_kf_list_ok(const orbfe_map* m, int n, const int32_t* kf_slots) {
    if (n < 0 || (n && !kf_slots)) return false;
    for (int i = 0; i < n; ++i)
        if (!m->kf_ok(kf_slots[i])) return false;
    return true;
}

}  // namespace

extern "C" {

int orbfe_map_set_scale_factors(orbfe_map* m, int nlevels, const float* scale) {
    if (!m || nlevels < 1 || nlevels > kMapMaxLevels || !scale) return ORBFE_ERR_ARG;
    return map_guarded(m, [&]() {
        int st;
        if ((st = m->scale.ensure(sizeof(float) * kMapMaxLevels))) return st;
        ORBFE_HIP(hipMemcpyAsync(m->scale.p, scale, sizeof(float) * (size_t)nlevels, hipMemcpyHostToDevice, m->stream));
        ORBFE_HIP(hipStreamSynchronize(m->stream));
        m->h_scale.assign(scale, scale + nlevels);
        return (int)ORBFE_OK;
    });
}

int orbfe_map_get_scale_factors(const orbfe_map* m, float* scale, int cap, int32_t* nlevels) {
    if (!m || !nlevels || cap < 0 || (cap && !scale)) return ORBFE_ERR_ARG;
    *nlevels = (int)m->h_scale.size();
    if (*nlevels > cap) return ORBFE_ERR_CAPACITY;
    if (*nlevels) std::memcpy(scale, m->h_scale.data(), sizeof(float) * m->h_scale.size());
    return ORBFE_OK;
}

int orbfe_map_set_keyframe_centers(orbfe_map* m, int n, const int32_t* kf_slots, const float* ow) {
    if (!m || !refresh_kf_list_ok(m, n, kf_slots) || (n && !ow)) return ORBFE_ERR_ARG;
    return map_guarded(m, [&]() {
        int st;
        if ((st = ref_ready_kf(m))) return st;
        return store_set<MapVec3>(m, m->at<MapVec3>(kColCenter), n, kf_slots, reinterpret_cast<const MapVec3*>(ow));
    });
}

int orbfe_map_get_keyframe_centers(orbfe_map* m, int n, const int32_t* kf_slots, float* ow) {
    if (!m || !refresh_kf_list_ok(m, n, kf_slots) || (n && !ow)) return ORBFE_ERR_ARG;
    return map_guarded(m, [&]() {
        int st;
        if ((st = ref_ready_kf(m))) return st;
        return store_get<MapVec3>(m, m->at<MapVec3>(kColCenter), n, kf_slots, reinterpret_cast<MapVec3*>(ow));
    });
}

static int refresh_set_descriptors(orbfe_map* m, int slot, int n, const uint8_t* desc, hipMemcpyKind kind) {
    if (!m || !m->kf_ok(slot) || n != m->kf_mp.len[slot] || (n && !desc)) return ORBFE_ERR_ARG;
    return map_guarded(m, [&]() {
        int st;
        if ((st = ref_ready_kf(m))) return st;
        if ((st = store_desc_pool(m))) return st;
        if (n)
            ORBFE_HIP(hipMemcpyAsync(m->kdesc_pool.buf.as<uint8_t>() + (size_t)kMapDescBytes * (size_t)m->kf_mp.off[slot],
                                     desc, (size_t)kMapDescBytes * (size_t)n, kind, m->stream));
        const int32_t s = slot;
        if ((st = store_set<uint8_t>(m, m->at<uint8_t>(kColDescSet), 1, &s, nullptr, 1))) return st;
        m->h_desc_set[slot] = 1;
        return (int)ORBFE_OK;
    });
}

int orbfe_map_set_keyframe_descriptors(orbfe_map* m, int slot, int n, const uint8_t* desc) {
    return refresh_set_descriptors(m, slot, n, desc, hipMemcpyHostToDevice);
}

int orbfe_map_set_keyframe_descriptors_device(orbfe_map* m, int slot, int n, const uint8_t* d_desc) {
    return refresh_set_descriptors(m, slot, n, d_desc, hipMemcpyDeviceToDevice);
}

int orbfe_map_get_keyframe_descriptors(orbfe_map* m, int slot, int cap, uint8_t* desc, int32_t* n,
                                       int32_t* is_set) {
    if (!m || !n || cap < 0 || (cap && !desc) || !m->kf_ok(slot)) return ORBFE_ERR_ARG;
    return map_guarded(m, [&]() {
        int st;
        if ((st = ref_ready_kf(m))) return st;
        if ((st = store_desc_pool(m))) return st;
        *n = m->kf_mp.len[slot];
        if (is_set) *is_set = m->h_desc_set[slot];
        if (*n > cap) return (int)ORBFE_ERR_CAPACITY;
        if (!*n) return (int)ORBFE_OK;
        ORBFE_HIP(hipMemcpyAsync(desc, m->kdesc_pool.buf.as<uint8_t>() + (size_t)kMapDescBytes * (size_t)m->kf_mp.off[slot],
                                 (size_t)kMapDescBytes * (size_t)*n, hipMemcpyDeviceToHost, m->stream));
        ORBFE_HIP(hipStreamSynchronize(m->stream));
        return (int)ORBFE_OK;
    });
}

int orbfe_map_set_point_ref_keyframes(orbfe_map* m, int n, const int32_t* mp_slots, const int32_t* kf_slots) {
    if (!m || n < 0 || (n && (!mp_slots || !kf_slots))) return ORBFE_ERR_ARG;
    for (int i = 0; i < n; ++i)
        if (!m->mp_ok(mp_slots[i]) || (kf_slots[i] != -1 && !m->kf_ok(kf_slots[i]))) return ORBFE_ERR_ARG;
    return map_guarded(m, [&]() {
        int st;
        if ((st = ref_ready_mp(m))) return st;
        return store_set<int>(m, m->at<int>(kColRefKf), n, mp_slots, kf_slots);
    });
}

int orbfe_map_get_point_ref_keyframes(orbfe_map* m, int n, const int32_t* mp_slots, int32_t* kf_slots) {
    if (!m || n < 0 || (n && (!mp_slots || !kf_slots))) return ORBFE_ERR_ARG;
    for (int i = 0; i < n; ++i)
        if (!m->mp_ok(mp_slots[i])) return ORBFE_ERR_ARG;
    return map_guarded(m, [&]() {
        int st;
        if ((st = ref_ready_mp(m))) return st;
        return store_get<int>(m, m->at<int>(kColRefKf), n, mp_slots, kf_slots);
    });
}

int orbfe_map_refresh_points_device(orbfe_map* m, int what, int n, const int32_t* d_list,
                                    const orbfe_map_point_arrays* arrays, uint8_t* d_result) {
    if (!refresh_args_ok(m, what, n, d_list, arrays)) return ORBFE_ERR_ARG;
    if (!n) return ORBFE_OK;
    return map_guarded(m, [&]() { return refresh_run(m, what, n, d_list, *arrays, d_result, nullptr); });
}

int orbfe_map_refresh_points(orbfe_map* m, int what, int n, const int32_t* mp_slots,
                             const orbfe_map_point_arrays* arrays, uint8_t* result) {
    if (!refresh_args_ok(m, what, n, mp_slots, arrays)) return ORBFE_ERR_ARG;
    if (!n) return ORBFE_OK;
    return map_guarded(m, [&]() {
        int st;
        int* d_list;
        if ((st = store_pin_reserve(m, ((size_t)n + 3) / 4))) return st;
        if ((st = store_stage_slots(m, n, mp_slots, d_list))) return st;
        // the masks come back through the pinned block's tail: one wait, on the done word
        st = refresh_run(m, what, n, d_list, *arrays, reinterpret_cast<uint8_t*>(m->pin_dev + kResTail), nullptr);
        if ((st == ORBFE_OK || st == ORBFE_ERR_UNSUPPORTED) && result) std::memcpy(result, m->pin + kResTail, (size_t)n);
        return st;
    });
}

int orbfe_map_refresh_keyframe_points(orbfe_map* m, int kf_slot, int what, const orbfe_map_point_arrays* arrays,
                                      int32_t* n_refreshed) {
    if (!m || !m->kf_ok(kf_slot)) return ORBFE_ERR_ARG;
    const int n = m->kf_mp.len[kf_slot];
    int dummy = 0;
    if (!refresh_args_ok(m, what, n, &dummy, arrays)) return ORBFE_ERR_ARG;
    if (n_refreshed) *n_refreshed = 0;
    if (!n) return ORBFE_OK;
    return map_guarded(m, [&]() {
        int live = 0;
        // the keyframe's mvpMapPoints where it lies: rows of kf_mp never move
        const int st = refresh_run(m, what, n, m->kf_mp_pool.buf.as<int>() + m->kf_mp.off[kf_slot], *arrays,
                                   nullptr, &live);
        if (n_refreshed) *n_refreshed = live;
        return st;
    });
}

int orbfe_map_process_new_keyframe(orbfe_map* m, int kf_slot, const orbfe_map_point_arrays* arrays,
                                   int32_t* recent, int recent_cap, int32_t* n_recent) {
    if (!m || !m->kf_ok(kf_slot) || !n_recent || recent_cap < 0 || (recent_cap && !recent)) return ORBFE_ERR_ARG;
    const int ns = m->kf_mp.len[kf_slot];
    int dummy = 0;
    if (!refresh_args_ok(m, ORBFE_MAP_REFRESH_NORMAL_DEPTH | ORBFE_MAP_REFRESH_DESCRIPTOR, ns, &dummy, arrays))
        return ORBFE_ERR_ARG;
    *n_recent = 0;
    if (!ns) return ORBFE_OK;
    return map_guarded(m, [&]() {
        int st;
        if ((st = store_pin_reserve(m, 2 * (size_t)ns))) return st;
        int* res = m->pin;
        __atomic_store_n(&res[kResDone], -1, __ATOMIC_RELEASE);
        hipLaunchKernelGGL(refresh_classify_kernel, dim3((unsigned)((ns + kRefBlock - 1) / kRefBlock)), dim3(kRefBlock),
                           0, m->stream, m->dev(), kf_slot, m->pin_dev + kResTail, m->pin_dev);
        ORBFE_HIP(hipGetLastError());
        if ((st = wait_words(res + kResDone, 1, -1, m->stream, 20000))) return st;
        const int* out = m->pin + kResTail;
        std::vector<int> add_mp, add_kf, add_ix, rec;
        std::unordered_set<int> seen;
        for (int i = 0; i < ns; ++i) {
            const int mp = out[2 * i], cls = out[2 * i + 1];
            if (!cls) continue;                                  // :145, :147
            if (!m->mp_ok(mp)) return (int)ORBFE_ERR_HIP;
            if (cls == 2 || !seen.insert(mp).second) {           // IsInKeyFrame (:149): by now it is
                rec.push_back(mp);                               // :157
                continue;
            }
            add_mp.push_back(mp);                                // :151
            add_kf.push_back(kf_slot);
            add_ix.push_back(i);
        }
        *n_recent = (int)rec.size();
        if (*n_recent > recent_cap) return (int)ORBFE_ERR_CAPACITY;
        if (!rec.empty()) std::memcpy(recent, rec.data(), sizeof(int) * rec.size());
        const int na = (int)add_mp.size();
        if (!na) return (int)ORBFE_OK;
        // what the refresh below would refuse is found before anything is added: the new
        // observer's descriptors, then a check launch over the points as they stand
        constexpr int kBoth = ORBFE_MAP_REFRESH_NORMAL_DEPTH | ORBFE_MAP_REFRESH_DESCRIPTOR;
        if ((st = ref_ready_kf(m))) return st;
        if (!m->h_desc_set[kf_slot]) return (int)ORBFE_ERR_ARG;
        int* d_add;
        if ((st = store_stage_slots(m, na, add_mp.data(), d_add))) return st;
        if ((st = refresh_run(m, kBoth, na, d_add, *arrays, nullptr, nullptr, 1))) return st;
        if ((st = orbfe_map_add_observations_idx(m, na, add_mp.data(), add_kf.data(), add_ix.data()))) return st;
        // :152-153 of every point added; a point's refresh reads its own observers only, so the
        // batch after the adds is the loop's sequence
        return orbfe_map_refresh_points(m, ORBFE_MAP_REFRESH_NORMAL_DEPTH | ORBFE_MAP_REFRESH_DESCRIPTOR, na,
                                        add_mp.data(), arrays, nullptr);
    });
}

}  // extern "C"
