// orbfe_localmap.hip — Tracking::UpdateLocalMap (Tracking.cc:1455-1599): the local keyframes and
// the local map points of a frame, from a device-resident mirror of the part of the map graph the
// two functions read, so that the chain SearchByProjection(last frame) -> local map ->
// SearchLocalPoints stays on the device.
//
//   map_vote_kernel      one wave per holder (frame keypoint), lanes striding the observations of
//                        the point it holds: integer counts per keyframe, the voted keyframes
//                        appended to a touched list on 0 -> 1, bad points NULLed (:1495-1511)
//   map_local_kf_kernel  one workgroup: the voted keyframes sorted by order key ("pointer order",
//                        DESIGN.md H26), phase 1 (:1523-1538) as a scan compaction plus a
//                        reduction to (max count, lowest position), phase 2 (:1542-1592) walked by
//                        one wave, the reference keyframe (:1594-1598)
//   map_mark_kernel      UpdateLocalPoints (:1465-1488): atomicMin of (rank, slot) per eligible point
//   map_count_kernel     per-block counts of the first occurrences; the last workgroup scans them
//   map_write_kernel     the ordered point list, the points' stamps, the done word
//   map_gather_kernel    the listed points' data into the contiguous inputs of
//                        orbfe_search_local_points_device
//   map_kf_key_kernel / map_neigh_kernel   a new keyframe's key, an assigned neighbour list
//
// The handle, its columns, row tables and staging are the store's (orbfe_map_store.hip); the
// mutators here go through store_put_rows, store_set and store_get.
//
// Everything is integer-exact.  The vote counts are deterministic; the touched list's order is
// not, and is used only as a set (it is sorted by key before anything reads it as an order).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <unordered_map>
#include <vector>

#include "../../include/orbfe.h"
#include "orbfe_device.hpp"

namespace orbfe {

constexpr int kMapLimit = 80;                            // :1545
constexpr int kMapMaxRankBlocks = 256;
constexpr int kResList = kResTail;                       // the keyframe list, in the pinned block's tail

// True in every thread of the last of the grid's `nblocks` workgroups (any grid shape) to get
// here; *counter is 0 before the launch.  The form of bow_pair_search (orbfe_bow.hip): barrier,
// then thread 0 fences and counts the workgroup — a fence in every wave ahead of the barrier, as
// last_workgroup() (orbfe_grid.hip) has it, cost these kernels 30 us each behind the scattered
// stores of 45,000 points (profiles/local_map/).
__device__ __forceinline__ bool map_last_workgroup(int* counter, int nblocks) {
    __shared__ int last;
    __syncthreads();
    if (threadIdx.x == 0) {
        __threadfence();
        last = atomicAdd(counter, 1) == nblocks - 1;
    }
    __syncthreads();
    if (!last) return false;
    __threadfence();
    return true;
}

// The counting loop of UpdateLocalKeyFrames (:1495-1511).  `holder_mp[i]` is the point slot held
// by holder i, or -1; nothing here assumes the holders are a frame's keypoints.
struct MapVoteArgs {
    MapDev d;
    int n;
    int* holder_mp;
};

__global__ __launch_bounds__(kMapBlock) void map_vote_kernel(MapVoteArgs a) {
    const MapDev& d = a.d;
    const int i = blockIdx.x * (kMapBlock / 64) + (threadIdx.x >> 6);
    if (i >= a.n) return;
    const int lane = threadIdx.x & 63;
    const int mp = a.holder_mp[i];
    if (mp == -1) return;
    if (mp < -1 || mp >= d.n_mp) {
        if (lane == 0) atomicOr(&d.ctl[kCtlErr], 1);
        return;
    }
    if (d.mp_bad[mp]) {  // :1508
        if (lane == 0) a.holder_mp[i] = -1;
        return;
    }
    const long long off = d.mp_obs_off[mp];
    const int no = d.mp_obs_n[mp];
    for (int j = lane; j < no; j += 64) {
        const int kf = d.mp_obs[off + j];
        if (kf < 0 || kf >= d.n_kf) continue;
        if (atomicAdd(&d.kf_cnt[kf], 1) == 0) {
            const int pos = atomicAdd(&d.ctl[kCtlTouched], 1);
            if (pos < kMapMaxVoted) d.touched[pos] = kf;
        }
    }
}

struct MapQueryArgs {
    MapDev d;
    unsigned long long frame_id;
    int* result;  // device-mapped pinned: kRes*
};

__device__ __forceinline__ unsigned long long map_ld_stamp(const unsigned long long* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(kMapBlock) void map_local_kf_kernel(MapQueryArgs a) {
    __shared__ unsigned long long keys[kMapMaxVoted];
    __shared__ int order[kMapMaxVoted];
    __shared__ int tmp[kMapBlock / 64 + 1];
    __shared__ unsigned long long s_best;
    __shared__ int s_size;
    const MapDev& d = a.d;
    const int tid = threadIdx.x;
    const int nt = d.ctl[kCtlTouched], err = d.ctl[kCtlErr];
    const int old_n = d.ctl[kCtlNKf];
    __syncthreads();
    if (err || nt > kMapMaxVoted) {
        // refused before any stamp, list or reference keyframe is written; the touched list is
        // incomplete here, so every counter is cleared
        for (int s = tid; s < d.n_kf; s += kMapBlock) d.kf_cnt[s] = 0;
        if (tid == 0) {
            d.ctl[kCtlTouched] = 0;
            d.ctl[kCtlErr] = 0;
            d.ctl[kCtlRun] = 0;
            d.ctl[kCtlStatus] = err ? ORBFE_ERR_ARG : ORBFE_ERR_CAPACITY;
            a.result[kResNKf] = err ? 0 : nt;
            a.result[kResRef] = d.ctl[kCtlRef];
        }
        return;
    }
    int n_list = old_n;  // :1513: an empty vote keeps the previous list and reference keyframe
    if (nt > 0) {
        int P = 1;
        while (P < nt) P <<= 1;
        for (int t = tid; t < P; t += kMapBlock) keys[t] = t < nt ? d.kf_key[d.touched[t]] : ~0ull;
        if (tid == 0) s_best = 0;
        __syncthreads();
        bitonic_sort_u64(keys, P);
        for (int t = tid; t < nt; t += kMapBlock) {
            const int slot = d.touched[t];
            const unsigned long long key = d.kf_key[slot];
            int lo = 0, hi = nt;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (keys[mid] < key) lo = mid + 1;
                else hi = mid;
            }
            order[lo] = slot;
        }
        __syncthreads();
        // phase 1 (:1523-1538), in key order: bad keyframes are neither listed, stamped nor
        // eligible; the first strict maximum is the largest count at the lowest position
        int base = 0;
        for (int c = 0; c < nt; c += kMapBlock) {
            const int e = c + tid;
            const int slot = e < nt ? order[e] : 0;
            const bool keep = e < nt && !d.kf_bad[slot];
            int total;
            const int ex = block_exclusive_scan<kMapBlock>(keep ? 1 : 0, tmp, total);
            if (keep) {
                d.local_kf[base + ex] = slot;
                d.kf_stamp[slot] = a.frame_id;
                const unsigned cnt = (unsigned)d.kf_cnt[slot];
                atomicMax(&s_best, ((unsigned long long)cnt << 32) | (unsigned)(0x7fffffff - e));
            }
            base += total;
        }
        __threadfence();
        __syncthreads();
        for (int t = tid; t < nt; t += kMapBlock) d.kf_cnt[d.touched[t]] = 0;
        const int n1 = base;
        // phase 2 (:1542-1592): sequential, one wave; only the phase-1 entries are visited
        if (tid < 64) {
            const int lane = tid;
            int size = n1;
            for (int it = 0; it < n1; ++it) {
                if (size > kMapLimit) break;  // :1545
                const int kf = d.local_kf[it];
                int pushed = -1;
                {   // the first neighbour that is neither bad nor stamped (:1552-1564)
                    const int nb = lane < kMapNeigh ? d.kf_neigh[kf * kMapNeigh + lane] : -1;
                    const bool ok = nb >= 0 && nb < d.n_kf && !d.kf_bad[nb] &&
                                    map_ld_stamp(&d.kf_stamp[nb]) != a.frame_id;
                    const unsigned long long m = __ballot(ok);
                    if (m) pushed = __shfl(nb, __ffsll((long long)m) - 1, 64);
                }
                if (pushed >= 0) {
                    if (lane == 0) {
                        d.local_kf[size] = pushed;
                        d.kf_stamp[pushed] = a.frame_id;
                    }
                    ++size;
                    __threadfence();
                }
                // the first child, in key order (:1566-1579)
                const long long co = d.kf_ch_off[kf];
                const int cn = d.kf_ch_n[kf];
                pushed = -1;
                for (int c0 = 0; c0 < cn && pushed < 0; c0 += 64) {
                    const int ch = c0 + lane < cn ? d.kf_ch[co + c0 + lane] : -1;
                    const bool ok = ch >= 0 && ch < d.n_kf && !d.kf_bad[ch] &&
                                    map_ld_stamp(&d.kf_stamp[ch]) != a.frame_id;
                    const unsigned long long m = __ballot(ok);
                    if (m) pushed = __shfl(ch, __ffsll((long long)m) - 1, 64);
                }
                if (pushed >= 0) {
                    if (lane == 0) {
                        d.local_kf[size] = pushed;
                        d.kf_stamp[pushed] = a.frame_id;
                    }
                    ++size;
                    __threadfence();
                }
                // the parent, with no isBad test; its break leaves the whole loop (:1581-1590)
                const int p = d.kf_parent[kf];
                if (p >= 0 && p < d.n_kf && map_ld_stamp(&d.kf_stamp[p]) != a.frame_id) {
                    if (lane == 0) {
                        d.local_kf[size] = p;
                        d.kf_stamp[p] = a.frame_id;
                    }
                    ++size;
                    __threadfence();
                    break;
                }
            }
            if (lane == 0) s_size = size;
        }
        __syncthreads();
        n_list = s_size;
        if (tid == 0 && s_best) d.ctl[kCtlRef] = order[0x7fffffff - (int)(unsigned)(s_best & 0xffffffffu)];
    }
    __threadfence();
    __syncthreads();
    for (int t = tid; t < n_list; t += kMapBlock) a.result[kResList + t] = d.local_kf[t];
    if (tid == 0) {
        d.ctl[kCtlTouched] = 0;
        d.ctl[kCtlNKf] = n_list;
        d.ctl[kCtlRun] = n_list;
        d.ctl[kCtlStatus] = ORBFE_OK;
        a.result[kResNKf] = n_list;
        a.result[kResRef] = d.ctl[kCtlRef];
    }
}

// UpdateLocalPoints (:1465-1488).  Workgroup (x, y) takes slots [1024 x, 1024 x + 1024) of the
// local keyframes of rank y, y + gridDim.y, ...; a position is rank * 8192 + slot.
__device__ __forceinline__ int map_slot_point(const MapDev& d, int rank, int slot) {
    const int kf = d.local_kf[rank];
    if (slot >= d.kf_mp_n[kf]) return -1;
    const int mp = d.kf_mp[d.kf_mp_off[kf] + slot];
    return mp >= 0 && mp < d.n_mp ? mp : -1;
}

__global__ __launch_bounds__(kMapBlock) void map_mark_kernel(MapQueryArgs a) {
    const MapDev& d = a.d;
    const int n_list = d.ctl[kCtlRun];
    const int slot = blockIdx.x * kMapBlock + threadIdx.x;
    for (int rank = blockIdx.y; rank < n_list; rank += gridDim.y) {
        const int mp = map_slot_point(d, rank, slot);
        if (mp < 0) continue;
        if (d.mp_stamp[mp] == a.frame_id || d.mp_bad[mp]) continue;  // :1479, :1481
        atomicMin(&d.first_pos[mp], rank * kMapMaxSlots + slot);
    }
}

__global__ __launch_bounds__(kMapBlock) void map_count_kernel(MapQueryArgs a) {
    __shared__ int tmp[kMapBlock / 64 + 1];
    const MapDev& d = a.d;
    const int tid = threadIdx.x;
    const int n_list = d.ctl[kCtlRun];
    const int slot = blockIdx.x * kMapBlock + tid;
    for (int rank = blockIdx.y; rank < n_list; rank += gridDim.y) {
        const int mp = map_slot_point(d, rank, slot);
        const int win = mp >= 0 && d.first_pos[mp] == rank * kMapMaxSlots + slot;
        const int total = block_sum<kMapBlock>(win, tmp);
        if (tid == 0) d.blk[rank * gridDim.x + blockIdx.x] = total;
    }
    if (!map_last_workgroup(&d.ctl[kCtlCountA], gridDim.x * gridDim.y)) return;
    const int nb = n_list * gridDim.x;
    int base = 0;
    for (int c = 0; c < nb; c += kMapBlock) {
        const int i = c + tid;
        const int v = i < nb ? d.blk[i] : 0;
        int total;
        const int ex = block_exclusive_scan<kMapBlock>(v, tmp, total);
        if (i < nb) d.blk[i] = base + ex;
        base += total;
    }
    if (tid == 0) {
        d.ctl[kCtlCountA] = 0;
        if (d.ctl[kCtlStatus] == ORBFE_OK) d.ctl[kCtlNMp] = base;
    }
}

__global__ __launch_bounds__(kMapBlock) void map_write_kernel(MapQueryArgs a) {
    __shared__ int tmp[kMapBlock / 64 + 1];
    const MapDev& d = a.d;
    const int tid = threadIdx.x;
    const int n_list = d.ctl[kCtlRun];
    const int slot = blockIdx.x * kMapBlock + tid;
    for (int rank = blockIdx.y; rank < n_list; rank += gridDim.y) {
        const int mp = map_slot_point(d, rank, slot);
        const int win = mp >= 0 && d.first_pos[mp] == rank * kMapMaxSlots + slot;
        int total;
        const int ex = block_exclusive_scan<kMapBlock>(win, tmp, total);
        if (win) {
            d.local_mp[d.blk[rank * gridDim.x + blockIdx.x] + ex] = mp;
            d.mp_stamp[mp] = a.frame_id;  // :1484
            d.first_pos[mp] = kMapNoPos;
        }
    }
    if (!map_last_workgroup(&d.ctl[kCtlCountB], gridDim.x * gridDim.y)) return;
    if (tid == 0) {
        d.ctl[kCtlCountB] = 0;
        a.result[kResNMp] = d.ctl[kCtlNMp];
        a.result[kResStatus] = d.ctl[kCtlStatus];
        __hip_atomic_store(&a.result[kResDone], 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// Four threads per listed point: descriptor halves; xyz + min distance; normal + max distance and
// the scalars.  A list entry outside the map is written as a bad point with id -1.
struct MapGatherArgs {
    int n, n_mp;
    const int* list;
    const uint8_t* mp_bad;
    orbfe_map_point_arrays src, dst;
};

__global__ __launch_bounds__(256) void map_gather_kernel(MapGatherArgs a) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    const int i = t >> 2, part = t & 3;
    if (i >= a.n) return;
    const int mp = a.list[i];
    const bool ok = mp >= 0 && mp < a.n_mp;
    const size_t s = ok ? (size_t)mp : 0;
    if (part < 2) {
        const uint4 v = ok ? reinterpret_cast<const uint4*>(a.src.desc)[2 * s + part] : make_uint4(0, 0, 0, 0);
        reinterpret_cast<uint4*>(a.dst.desc)[2 * (size_t)i + part] = v;
    } else if (part == 2) {
        for (int k = 0; k < 3; ++k) a.dst.xyz[3 * (size_t)i + k] = ok ? a.src.xyz[3 * s + k] : 0.f;
        a.dst.min_dist[i] = ok ? a.src.min_dist[s] : 0.f;
    } else {
        for (int k = 0; k < 3; ++k) a.dst.normal[3 * (size_t)i + k] = ok ? a.src.normal[3 * s + k] : 0.f;
        a.dst.max_dist[i] = ok ? a.src.max_dist[s] : 0.f;
        a.dst.n_obs[i] = ok ? a.src.n_obs[s] : 0;
        a.dst.skip[i] = ok ? a.src.skip[s] : 1;
        a.dst.mp_ids[i] = ok ? mp : -1;
        a.dst.bad[i] = ok ? a.mp_bad[s] : 1;
    }
}

struct MapNeighList {
    int v[kMapNeigh];
};

// A new KeyFrame's key; everything else of it is at the columns' defaults (kMapColumns).
__global__ void map_kf_key_kernel(int slot, unsigned long long key, unsigned long long* kf_key) {
    if (threadIdx.x == 0) kf_key[slot] = key;
}

__global__ void map_neigh_kernel(int slot, MapNeighList l, int* kf_neigh) {
    if (threadIdx.x < kMapNeigh) kf_neigh[slot * kMapNeigh + threadIdx.x] = l.v[threadIdx.x];
}

}  // namespace orbfe

using namespace orbfe;

namespace {

// The five launches of one query over the device array d_frame_mp; waits on the done word.
int map_query(orbfe_map* m, uint64_t frame_id, int n, int32_t* d_frame_mp) {
    int* res = m->pin;
    res[kResNKf] = res[kResNMp] = 0;
    res[kResStatus] = ORBFE_OK;
    __atomic_store_n(&res[kResDone], -1, __ATOMIC_RELEASE);
    const MapDev d = m->dev();
    if (n > 0) {
        MapVoteArgs v{d, n, d_frame_mp};
        const int per = kMapBlock / 64;
        hipLaunchKernelGGL(map_vote_kernel, dim3((n + per - 1) / per), dim3(kMapBlock), 0, m->stream, v);
    }
    MapQueryArgs q{d, frame_id, m->pin_dev};
    hipLaunchKernelGGL(map_local_kf_kernel, dim3(1), dim3(kMapBlock), 0, m->stream, q);
    // the list's length is known on the device only: the point kernels stride over the ranks
    const int bound = std::max((int)m->h_local.size(), std::min(m->n_kf, kMapMaxVoted) + 3);
    const dim3 grid(std::max(1, (m->max_slots + kMapBlock - 1) / kMapBlock),
                    std::max(1, std::min(bound, kMapMaxRankBlocks)));
    hipLaunchKernelGGL(map_mark_kernel, grid, dim3(kMapBlock), 0, m->stream, q);
    hipLaunchKernelGGL(map_count_kernel, grid, dim3(kMapBlock), 0, m->stream, q);
    hipLaunchKernelGGL(map_write_kernel, grid, dim3(kMapBlock), 0, m->stream, q);
    if (hipGetLastError() != hipSuccess) return ORBFE_ERR_HIP;
    int st;
    if ((st = wait_words(res + kResDone, 1, -1, m->stream, 20000))) return st;
    if (res[kResStatus] == ORBFE_OK) {
        m->h_local.assign(res + kResList, res + kResList + res[kResNKf]);
        m->h_ref = res[kResRef];
        m->h_n_local_mp = res[kResNMp];
    }
    return res[kResStatus];
}

}  // namespace

extern "C" {

int orbfe_map_add_keyframe(orbfe_map* m, uint64_t order_key, int n_slots, const int32_t* mp_slots,
                           int32_t* slot) {
    if (!m || !slot || n_slots < 0 || n_slots > kMapMaxSlots || m->by_key.count(order_key))
        return ORBFE_ERR_ARG;
    if (mp_slots)
        for (int i = 0; i < n_slots; ++i)
            if (mp_slots[i] != -1 && !m->mp_ok(mp_slots[i])) return ORBFE_ERR_ARG;
    return map_guarded(m, [&]() {
        int st;
        const int s = m->n_kf;
        if ((st = store_cover(m, kGroupCoreKf, s + 1, 16))) return st;
        hipLaunchKernelGGL(map_kf_key_kernel, dim3(1), dim3(64), 0, m->stream, s,
                           (unsigned long long)order_key, m->at<unsigned long long>(kColKfKey));
        ORBFE_HIP(hipGetLastError());
        std::vector<int> none;
        if (!mp_slots) none.assign((size_t)n_slots, -1);
        if ((st = map_put_kf_mp(m, {{s, 0, n_slots, n_slots, mp_slots ? mp_slots : none.data(), nullptr}})))
            return st;
        m->h_key.push_back(order_key);
        m->by_key[order_key] = s;
        m->max_slots = std::max(m->max_slots, n_slots);
        ++m->n_kf;
        *slot = s;
        return (int)ORBFE_OK;
    });
}

int orbfe_map_set_keyframe_points(orbfe_map* m, int slot, int first, int n, const int32_t* mp_slots) {
    if (!m || !m->kf_ok(slot) || first < 0 || n < 0 || (n && !mp_slots) ||
        (long long)first + n > m->kf_mp.len[slot])
        return ORBFE_ERR_ARG;
    for (int i = 0; i < n; ++i)
        if (mp_slots[i] != -1 && !m->mp_ok(mp_slots[i])) return ORBFE_ERR_ARG;
    if (!n) return ORBFE_OK;
    return map_guarded(m, [&]() { return map_put_kf_mp(m, {{slot, first, n, -1, mp_slots, nullptr}}); });
}

int orbfe_map_set_keyframe_bad(orbfe_map* m, int slot, int bad) {
    if (!m || !m->kf_ok(slot)) return ORBFE_ERR_ARG;
    return map_guarded(m, [&]() {
        const int32_t s = slot;
        return store_set<uint8_t>(m, m->at<uint8_t>(kColKfBad), 1, &s, nullptr, bad ? 1 : 0);
    });
}

int orbfe_map_set_covisibility(orbfe_map* m, int slot, int n, const int32_t* neigh_slots) {
    if (!m || !m->kf_ok(slot) || n < 0 || n > kMapNeigh || (n && !neigh_slots)) return ORBFE_ERR_ARG;
    MapNeighList l;
    for (int j = 0; j < kMapNeigh; ++j) {
        l.v[j] = j < n ? neigh_slots[j] : -1;
        if (l.v[j] != -1 && !m->kf_ok(l.v[j])) return ORBFE_ERR_ARG;
    }
    return map_guarded(m, [&]() {
        hipLaunchKernelGGL(map_neigh_kernel, dim3(1), dim3(64), 0, m->stream, slot, l, m->at<int>(kColKfNeigh));
        ORBFE_HIP(hipGetLastError());
        return (int)ORBFE_OK;
    });
}

int orbfe_map_set_children(orbfe_map* m, int slot, int n, const int32_t* child_slots) {
    if (!m || !m->kf_ok(slot) || n < 0 || (n && !child_slots)) return ORBFE_ERR_ARG;
    for (int i = 0; i < n; ++i)
        if (!m->kf_ok(child_slots[i])) return ORBFE_ERR_ARG;
    return map_guarded(m, [&]() {
        // std::set<KeyFrame*>: distinct, ascending key
        std::vector<int> c(child_slots, child_slots + n);
        std::sort(c.begin(), c.end(), [&](int x, int y) { return m->h_key[x] < m->h_key[y]; });
        c.erase(std::unique(c.begin(), c.end()), c.end());
        return map_put_kf_ch(m, {{slot, 0, (int)c.size(), (int)c.size(), c.data(), nullptr}});
    });
}

int orbfe_map_set_parent(orbfe_map* m, int slot, int parent) {
    if (!m || !m->kf_ok(slot) || (parent != -1 && !m->kf_ok(parent))) return ORBFE_ERR_ARG;
    return map_guarded(m, [&]() {
        const int32_t s = slot;
        return store_set<int>(m, m->at<int>(kColKfParent), 1, &s, nullptr, parent);
    });
}

int orbfe_map_add_points(orbfe_map* m, int n, int32_t* first_slot) {
    if (!m || n < 0 || !first_slot || (long long)m->n_mp + n > 0x7fffffff) return ORBFE_ERR_ARG;
    return map_guarded(m, [&]() {
        int st;
        // a new MapPoint is at the columns' defaults (kMapColumns)
        if ((st = store_cover(m, kGroupCoreMp, m->n_mp + n, 1024))) return st;
        *first_slot = m->n_mp;
        m->n_mp += n;
        m->h_obs.resize((size_t)m->n_mp);
        m->h_idx.resize((size_t)m->n_mp);
        m->mp_obs.cover((size_t)m->n_mp);
        return (int)ORBFE_OK;
    });
}

int orbfe_map_set_points_bad(orbfe_map* m, int n, const int32_t* mp_slots, int bad) {
    if (!m || n < 0 || (n && !mp_slots)) return ORBFE_ERR_ARG;
    for (int i = 0; i < n; ++i)
        if (!m->mp_ok(mp_slots[i])) return ORBFE_ERR_ARG;
    return map_guarded(m, [&]() {
        return store_set<uint8_t>(m, m->at<uint8_t>(kColMpBad), n, mp_slots, nullptr, bad ? 1 : 0);
    });
}

// MapPoint::AddObservation (MapPoint.cc:339-350) / the erase of EraseObservation (:357-365),
// batched.  idx = NULL: the index is not known (-1), nObs changes by 1.
static int map_change_observations(orbfe_map* m, int n, const int32_t* mp_slots,
                                   const int32_t* kf_slots, const int32_t* idx, bool add) {
    if (!m || n < 0 || (n && (!mp_slots || !kf_slots))) return ORBFE_ERR_ARG;
    for (int i = 0; i < n; ++i) {
        if (!m->mp_ok(mp_slots[i]) || !m->kf_ok(kf_slots[i])) return ORBFE_ERR_ARG;
        if (idx && (idx[i] < 0 || idx[i] >= m->kf_mp.len[kf_slots[i]])) return ORBFE_ERR_ARG;
    }
    return map_guarded(m, [&]() {
        int st;
        // mpRefKF of the points an erase may touch, once the column exists (MapPoint.cc:367-368)
        std::unordered_map<int, int> ref;
        std::vector<int> ref_changed;
        if (!add && n && ref_made(m)) {
            if ((st = ref_ready_mp(m))) return st;
            std::vector<int> r((size_t)n);
            if ((st = store_get<int>(m, m->at<int>(kColRefKf), n, mp_slots, r.data()))) return st;
            for (int i = 0; i < n; ++i) ref[mp_slots[i]] = r[i];
        }
        std::vector<int> dirty, who, amount;
        for (int i = 0; i < n; ++i) {
            std::vector<int>& o = m->h_obs[mp_slots[i]];
            std::vector<int>& x = m->h_idx[mp_slots[i]];
            auto it = std::lower_bound(o.begin(), o.end(), kf_slots[i]);
            const bool has = it != o.end() && *it == kf_slots[i];
            if (add == has) continue;  // set semantics (MapPoint.cc:342-343, :357)
            const auto xi = x.begin() + (it - o.begin());
            const int ix = add ? (idx ? idx[i] : -1) : *xi;
            const int by = ix >= 0 && map_has_right(m, kf_slots[i], ix) ? 2 : 1;  // :346-349, :360-363
            if (ix < 0) m->n_unknown += add ? 1 : -1;
            if (add) {
                o.insert(it, kf_slots[i]);
                x.insert(xi, ix);
            } else {
                o.erase(it);
                x.erase(xi);
                const auto r = ref.find(mp_slots[i]);
                if (r != ref.end() && r->second == kf_slots[i]) {
                    // mObservations.begin()->first: the lowest order key that remains, or -1
                    int next = -1;
                    for (int k : o)
                        if (next < 0 || m->h_key[k] < m->h_key[next]) next = k;
                    r->second = next;
                    ref_changed.push_back(mp_slots[i]);
                }
            }
            dirty.push_back(mp_slots[i]);
            who.push_back(mp_slots[i]);
            amount.push_back(add ? by : -by);
        }
        std::sort(dirty.begin(), dirty.end());
        dirty.erase(std::unique(dirty.begin(), dirty.end()), dirty.end());
        std::vector<MapRowWrite> w;
        for (int p : dirty) {
            const std::vector<int>& o = m->h_obs[p];
            w.push_back({p, 0, (int)o.size(), (int)o.size(), o.data(), m->h_idx[p].data()});
        }
        if ((st = map_put_mp_obs(m, w))) return st;
        if (!ref_changed.empty()) {
            std::sort(ref_changed.begin(), ref_changed.end());
            ref_changed.erase(std::unique(ref_changed.begin(), ref_changed.end()), ref_changed.end());
            std::vector<int> v;
            for (int p : ref_changed) v.push_back(ref[p]);
            if ((st = store_set<int>(m, m->at<int>(kColRefKf), (int)v.size(), ref_changed.data(), v.data())))
                return st;
        }
        if ((st = cull_ready(m))) return st;
        return store_add(m, m->at<int>(kColNobs), (int)who.size(), who.data(), amount.data());
    });
}

int orbfe_map_add_observations(orbfe_map* m, int n, const int32_t* mp_slots, const int32_t* kf_slots) {
    return map_change_observations(m, n, mp_slots, kf_slots, nullptr, true);
}

int orbfe_map_add_observations_idx(orbfe_map* m, int n, const int32_t* mp_slots, const int32_t* kf_slots,
                                   const int32_t* idx) {
    if (n > 0 && !idx) return ORBFE_ERR_ARG;
    return map_change_observations(m, n, mp_slots, kf_slots, idx, true);
}

int orbfe_map_erase_observations(orbfe_map* m, int n, const int32_t* mp_slots, const int32_t* kf_slots) {
    return map_change_observations(m, n, mp_slots, kf_slots, nullptr, false);
}

int orbfe_map_set_stamps(orbfe_map* m, int kind, int n, const int32_t* slots, const uint64_t* stamps) {
    if (!m || (kind != ORBFE_MAP_KEYFRAMES && kind != ORBFE_MAP_POINTS) || n < 0 ||
        (n && (!slots || !stamps)))
        return ORBFE_ERR_ARG;
    for (int i = 0; i < n; ++i)
        if (kind == ORBFE_MAP_KEYFRAMES ? !m->kf_ok(slots[i]) : !m->mp_ok(slots[i])) return ORBFE_ERR_ARG;
    return map_guarded(m, [&]() {
        return store_set<unsigned long long>(m, m->at<unsigned long long>(kind == ORBFE_MAP_KEYFRAMES ? kColKfStamp : kColMpStamp),
                                             n, slots, reinterpret_cast<const unsigned long long*>(stamps));
    });
}

int orbfe_map_get_stamps(orbfe_map* m, int kind, int n, const int32_t* slots, uint64_t* stamps) {
    if (!m || (kind != ORBFE_MAP_KEYFRAMES && kind != ORBFE_MAP_POINTS) || n < 0 ||
        (n && (!slots || !stamps)))
        return ORBFE_ERR_ARG;
    for (int i = 0; i < n; ++i)
        if (kind == ORBFE_MAP_KEYFRAMES ? !m->kf_ok(slots[i]) : !m->mp_ok(slots[i])) return ORBFE_ERR_ARG;
    if (!n) return ORBFE_OK;
    return map_guarded(m, [&]() {
        return store_get<unsigned long long>(m, m->at<unsigned long long>(kind == ORBFE_MAP_KEYFRAMES ? kColKfStamp : kColMpStamp),
                                             n, slots, reinterpret_cast<unsigned long long*>(stamps));
    });
}

int orbfe_map_set_local_keyframes(orbfe_map* m, int n, const int32_t* kf_slots, int ref_kf) {
    if (!m || n < 0 || n > kMapListCap || (n && !kf_slots) || (ref_kf != -1 && !m->kf_ok(ref_kf)))
        return ORBFE_ERR_ARG;
    for (int i = 0; i < n; ++i)
        if (!m->kf_ok(kf_slots[i])) return ORBFE_ERR_ARG;
    return map_guarded(m, [&]() {
        if (n)
            ORBFE_HIP(hipMemcpyAsync(m->local_kf.p, kf_slots, sizeof(int) * (size_t)n, hipMemcpyHostToDevice, m->stream));
        const int h[2] = {n, ref_kf};  // kCtlNKf, kCtlRef
        ORBFE_HIP(hipMemcpyAsync(m->ctl.as<int>() + kCtlNKf, h, sizeof h, hipMemcpyHostToDevice, m->stream));
        ORBFE_HIP(hipStreamSynchronize(m->stream));
        m->h_local.assign(kf_slots, kf_slots + n);
        m->h_ref = ref_kf;
        return (int)ORBFE_OK;
    });
}

int orbfe_map_get_local_keyframes(const orbfe_map* m, int32_t* kf_slots, int cap, int32_t* n,
                                  int32_t* ref_kf) {
    if (!m || !n || cap < 0 || (cap && !kf_slots)) return ORBFE_ERR_ARG;
    *n = (int)m->h_local.size();
    if (ref_kf) *ref_kf = m->h_ref;
    if (*n > cap) return ORBFE_ERR_CAPACITY;
    if (*n) std::memcpy(kf_slots, m->h_local.data(), sizeof(int) * (size_t)*n);
    return ORBFE_OK;
}

int orbfe_map_update_local_device(orbfe_map* m, uint64_t frame_id, int n, int32_t* d_frame_mp,
                                  int32_t* local_kf, int kf_cap, int32_t* n_local_kf,
                                  int32_t* ref_kf, int32_t* n_local_mp) {
    if (!m || n < 0 || (n && !d_frame_mp) || kf_cap < 0 || (kf_cap && !local_kf) || !n_local_kf ||
        !ref_kf || !n_local_mp)
        return ORBFE_ERR_ARG;
    return map_guarded(m, [&]() {
        const int st = map_query(m, frame_id, n, d_frame_mp);
        *n_local_kf = m->pin[kResNKf];
        *ref_kf = m->pin[kResRef];
        *n_local_mp = m->pin[kResNMp];
        if (st != ORBFE_OK) return st;
        if (*n_local_kf > kf_cap) return (int)ORBFE_ERR_CAPACITY;
        if (*n_local_kf) std::memcpy(local_kf, m->pin + kResList, sizeof(int) * (size_t)*n_local_kf);
        return (int)ORBFE_OK;
    });
}

int orbfe_map_update_local(orbfe_map* m, uint64_t frame_id, int n, int32_t* frame_mp,
                           int32_t* local_kf, int kf_cap, int32_t* n_local_kf, int32_t* ref_kf,
                           int32_t* local_mp, int mp_cap, int32_t* n_local_mp) {
    if (!m || n < 0 || (n && !frame_mp) || mp_cap < 0 || (mp_cap && !local_mp)) return ORBFE_ERR_ARG;
    for (int i = 0; i < n; ++i)
        if (frame_mp[i] != -1 && !m->mp_ok(frame_mp[i])) return ORBFE_ERR_ARG;
    if (kf_cap < 0 || (kf_cap && !local_kf) || !n_local_kf || !ref_kf || !n_local_mp) return ORBFE_ERR_ARG;
    return map_guarded(m, [&]() {
        int st;
        int* d_frame;  // the holders: the query borrows no staging
        if ((st = store_borrow(m, kStageSlots, (size_t)n, d_frame))) return st;
        if (n)
            ORBFE_HIP(hipMemcpyAsync(d_frame, frame_mp, sizeof(int) * (size_t)n, hipMemcpyHostToDevice, m->stream));
        st = orbfe_map_update_local_device(m, frame_id, n, d_frame, local_kf, kf_cap,
                                           n_local_kf, ref_kf, n_local_mp);
        if (st != ORBFE_OK && st != ORBFE_ERR_CAPACITY) return st;
        if (n) {  // the NULLed bad points (:1508), also next to ORBFE_ERR_CAPACITY
            ORBFE_HIP(hipMemcpyAsync(frame_mp, d_frame, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, m->stream));
            ORBFE_HIP(hipStreamSynchronize(m->stream));
        }
        if (st != ORBFE_OK) return st;
        if (*n_local_mp > mp_cap) return (int)ORBFE_ERR_CAPACITY;
        if (*n_local_mp) {
            ORBFE_HIP(hipMemcpyAsync(local_mp, m->at<int>(kColLocalMp), sizeof(int) * (size_t)*n_local_mp,
                                     hipMemcpyDeviceToHost, m->stream));
            ORBFE_HIP(hipStreamSynchronize(m->stream));
        }
        return (int)ORBFE_OK;
    });
}

int orbfe_map_local_points_device(const orbfe_map* m, const int32_t** d_list, int32_t* n) {
    if (!m || !d_list || !n) return ORBFE_ERR_ARG;
    *d_list = m->at<int32_t>(kColLocalMp);
    *n = m->h_n_local_mp;
    return ORBFE_OK;
}

int orbfe_map_get_local_points(orbfe_map* m, int32_t* mp_slots, int cap, int32_t* n) {
    if (!m || !n || cap < 0 || (cap && !mp_slots)) return ORBFE_ERR_ARG;
    *n = m->h_n_local_mp;
    if (*n > cap) return ORBFE_ERR_CAPACITY;
    if (!*n) return ORBFE_OK;
    return map_guarded(m, [&]() {
        ORBFE_HIP(hipMemcpyAsync(mp_slots, m->at<int>(kColLocalMp), sizeof(int) * (size_t)*n, hipMemcpyDeviceToHost, m->stream));
        ORBFE_HIP(hipStreamSynchronize(m->stream));
        return (int)ORBFE_OK;
    });
}

int orbfe_map_gather_points_device(orbfe_map* m, int n, const int32_t* d_list,
                                   const orbfe_map_point_arrays* src,
                                   const orbfe_map_point_arrays* dst) {
    if (!m || n < 0 || !src || !dst) return ORBFE_ERR_ARG;
    if (!n) return ORBFE_OK;
    if (!d_list || !src->xyz || !src->normal || !src->min_dist || !src->max_dist || !src->desc ||
        !src->n_obs || !src->skip || !dst->xyz || !dst->normal || !dst->min_dist || !dst->max_dist ||
        !dst->desc || !dst->n_obs || !dst->skip || !dst->mp_ids || !dst->bad ||
        ((uintptr_t)src->desc & 15) || ((uintptr_t)dst->desc & 15))
        return ORBFE_ERR_ARG;
    return map_guarded(m, [&]() {
        MapGatherArgs a{n, m->n_mp, d_list, m->at<uint8_t>(kColMpBad), *src, *dst};
        const long long threads = 4ll * n;
        hipLaunchKernelGGL(map_gather_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0,
                           m->stream, a);
        ORBFE_HIP(hipGetLastError());
        return (int)ORBFE_OK;
    });
}

}  // extern "C"
