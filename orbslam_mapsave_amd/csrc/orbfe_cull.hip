// orbfe_cull.hip — LocalMapping's culling on an orbfe_map: LocalMapping::MapPointCulling
// (LocalMapping.cc:170-205) and KeyFrameCulling (:632-698), KeyFrame::SetBadFlag complete and SetErase
// (KeyFrame.cc:1158-1287), MapPoint::AddObservation with its feature index / EraseObservation /
// SetBadFlag (MapPoint.cc:339-409), KeyFrame::TrackedMapPoints (KeyFrame.cc:971-996) and the state
// they read, DESIGN.md H28.
//
//   cull_points_kernel   one workgroup, one thread per listed point: the four branches of
//                        MapPointCulling, a repeated point resolved by its first position, the
//                        kept and the culled list written by order-preserving scans
//   cull_setbad_kernel   one wave per point: MapPoint::SetBadFlag (:392-409), lanes striding the
//                        observers; EraseMapPointMatch(idx) writes -1 whatever the entry held
//   cull_tracked_kernel  one workgroup: TrackedMapPoints over a keyframe's slots
//   cull_kf_obs_kernel   one wave per slot of a keyframe: EraseObservation(this) of what it holds, in
//                        three launches (marking, checking, applying), KeyFrame.cc:1191-1193
//   cull_kf_finish_kernel  one workgroup: what the erases did as ordered lists, the spanning-tree
//                        tournament (:1201-1274) over the children's lists and weight rows, mbBad
//   cull_decide_kernel   one workgroup per listed keyframe: nMPs and nRedundantObservations of
//                        KeyFrameCulling, waves over the slots, lanes over a point's observers
//   cull_add_masked_kernel   the counters' device-side mutator
//
// Per point: nObs (state: SetBadFlag clears the observations and leaves it), mnFound, mnVisible,
// mnFirstKFid.  Per observation: the feature index, in a side pool of the observation rows
// (orbfe_map::mp_idx_pool: same offsets, same lengths), so that the rows map_vote_kernel and
// cov_count_kernel read keep their layout.  Per keyframe keypoint: octave and `mvuRight >= 0` in
// one byte, mvDepth, in side pools of kf_mp.  The columns, pools and their views (CullDev) are
// the store's (orbfe_map_store.hip); cull_ready() there makes them cover the map.
// The host keeps the observation rows with their indices and the right flags, so every nObs
// amount and every "index unknown" refusal is decided before a kernel writes.  Everything is
// integer but the found ratio, one IEEE float division and one comparison.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "../../include/orbfe.h"
#include "orbfe_device.hpp"

namespace orbfe {

constexpr int kCullBlock = 1024;
constexpr int kCullNoPos = kMapNoPos;    // mark of a point no list position has claimed

// The device form: entries of -1 and entries whose mask byte is 0 are skipped.  Run twice:
// checking (an entry outside [-1, n_mp) raises *err, nothing written) and adding (nothing if *err).
__global__ __launch_bounds__(256) void cull_add_masked_kernel(int n, const int* slots, const uint8_t* mask,
                                                              int n_mp, int apply, int* dst, int* err) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int s = slots[i];
    if (!apply) {
        if (s < -1 || s >= n_mp) atomicOr(err, 1);
        return;
    }
    if (*err || s < 0 || s >= n_mp || (mask && !mask[i])) return;
    atomicAdd(&dst[s], 1);
}

struct CullPointsArgs {
    MapDev d;
    CullDev c;
    int n, th_obs;
    int cur;            // nCurrentKFid, in [0, 2^31)
    const int* list;    // [n] point slots, all in range
    int* kept;          // [n] device-mapped pinned
    int* culled;        // [n]
    int* res;           // the handle's pinned block
};

// LocalMapping.cc:183-204.  Changes nothing but the marks, which it puts back.
__global__ __launch_bounds__(kCullBlock) void cull_points_kernel(CullPointsArgs a) {
    __shared__ int tmp[kCullBlock / 64 + 1];
    __shared__ int s_err;
    const MapDev& d = a.d;
    const CullDev& cu = a.c;
    const int tid = threadIdx.x;
    if (tid == 0) s_err = 0;
    // a point listed twice: the second occurrence sees what the first one did
    for (int i = tid; i < a.n; i += kCullBlock) atomicMin(&cu.mark[a.list[i]], i);
    __threadfence();
    __syncthreads();
    int n_kept = 0, n_culled = 0;
    for (int c = 0; c < a.n; c += kCullBlock) {
        const int i = c + tid;
        int mp = 0;
        bool keep = false, bad = false;
        if (i < a.n) {
            mp = a.list[i];
            const bool first = __hip_atomic_load(&cu.mark[mp], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == i;
            if (!d.mp_bad[mp]) {                                                   // :186
                const float ratio = (float)cu.found[mp] / (float)cu.visible[mp];     // MapPoint.cc GetFoundRatio
                const long long f = cu.first_kf[mp];
                if (f < 0 || f > 0x7fffffffll) s_err = 1;
                const int diff = a.cur - (int)f;
                if (ratio < 0.25f) bad = true;                                     // :190
                else if (diff >= 2 && cu.nobs[mp] <= a.th_obs) bad = true;          // :195
                else if (diff >= 3) keep = false;                                  // :200
                else keep = true;
                if (bad && !first) bad = false;  // made bad at its first position: dropped here (:186)
            }
        }
        int total;
        const int ek = block_exclusive_scan<kCullBlock>(keep ? 1 : 0, tmp, total);
        if (keep) a.kept[n_kept + ek] = mp;
        n_kept += total;
        const int ec = block_exclusive_scan<kCullBlock>(bad ? 1 : 0, tmp, total);
        if (bad) a.culled[n_culled + ec] = mp;
        n_culled += total;
    }
    __syncthreads();
    for (int i = tid; i < a.n; i += kCullBlock) cu.mark[a.list[i]] = kCullNoPos;
    __threadfence_system();
    __syncthreads();
    if (tid == 0) {
        a.res[kResKept] = n_kept;
        a.res[kResCulled] = n_culled;
        a.res[kResCullStatus] = s_err ? ORBFE_ERR_ARG : ORBFE_OK;
        __hip_atomic_store(&a.res[kResDone], 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// MapPoint::SetBadFlag (MapPoint.cc:392-409) of n distinct points, one wave each.  nObs stays.
__global__ __launch_bounds__(256) void cull_setbad_kernel(MapDev d, int n, const int* slots) {
    const int w = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= n) return;
    const int lane = threadIdx.x & 63;
    const int mp = slots[w];
    if (mp < 0 || mp >= d.n_mp) return;
    const long long oo = d.mp_obs_off[mp];
    const int no = d.mp_obs_n[mp];
    for (int j = lane; j < no; j += 64) {
        const int kf = d.mp_obs[oo + j], ix = d.mp_idx[oo + j];
        if (kf < 0 || kf >= d.n_kf || ix < 0 || ix >= d.kf_mp_n[kf]) continue;
        d.kf_mp[d.kf_mp_off[kf] + ix] = -1;   // EraseMapPointMatch(idx), :405: whatever it held
    }
    if (lane == 0) {
        d.mp_bad[mp] = 1;                     // :398
        d.mp_obs_n[mp] = 0;                      // :400
    }
}

// KeyFrame::TrackedMapPoints (KeyFrame.cc:971-996).
__global__ __launch_bounds__(kCullBlock) void cull_tracked_kernel(MapDev d, CullDev cu, int kf, int min_obs, int* res) {
    __shared__ int tmp[kCullBlock / 64 + 1];
    const long long off = d.kf_mp_off[kf];
    const int n = d.kf_mp_n[kf];
    int cnt = 0;
    for (int i = threadIdx.x; i < n; i += kCullBlock) {
        const int mp = d.kf_mp[off + i];
        if (mp < 0 || mp >= d.n_mp) continue;      // :980
        if (d.mp_bad[mp]) continue;                // :982
        if (min_obs > 0 && cu.nobs[mp] < min_obs) continue;  // :984-987
        ++cnt;
    }
    const int total = block_sum<kCullBlock>(cnt, tmp);
    if (threadIdx.x == 0) {
        res[kResValue] = total;
        __hip_atomic_store(&res[kResDone], 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// ---- KeyFrame::SetBadFlag (KeyFrame.cc:1174-1287) and LocalMapping::KeyFrameCulling (:632-698)

constexpr int kCullWaves = kCullBlock / 64;
constexpr int kCullMaxList = ORBFE_MAP_MAX_CULL_LIST;
enum { kCullMark, kCullCheck, kCullApply };
enum { kCullOutErased, kCullOutBad, kCullOutRounds, kCullOutPairs, kCullOutParent, kCullOutLists };  // pinned words of a SetBadFlag

__device__ __forceinline__ int cull_ld(const int* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// mObservations.begin()->first once position p has left the row at oo: the remaining observer with
// the lowest order key (rows are stored by slot), or -1 where the reference dereferences begin()
// of an empty map.  The whole wave calls it; every lane returns the answer.
__device__ __forceinline__ int cull_first_observer(const MapDev& d, long long oo, int no, int p, int lane) {
    unsigned long long best = ~0ull;
    int who = -1;
    for (int j = lane; j < no; j += 64) {
        if (j == p) continue;
        const int kfj = d.mp_obs[oo + j];
        if (kfj < 0 || kfj >= d.n_kf) continue;
        const unsigned long long key = d.kf_key[kfj];
        if (who < 0 || key < best) {
            best = key;
            who = kfj;
        }
    }
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
        const unsigned long long ob = __shfl_xor(best, s, 64);
        const int ow = __shfl_xor(who, s, 64);
        if (ow >= 0 && (who < 0 || ob < best)) {
            best = ob;
            who = ow;
        }
    }
    return who;
}

// EraseObservation(this) of every entry of the keyframe's mvpMapPoints (:1191-1193), one wave per
// slot, in three launches: marking (a point held at two indices is erased at the lower one, the
// other finds nothing), checking (what each erase will do; a point that will go bad with an
// observer whose index is unknown raises *err; nothing written but flag[]) and applying (nothing
// if *err).  The writes of different waves are disjoint, or the same -1.
struct CullKfObsArgs {
    MapDev d;
    CullDev c;
    int kf, mode;
    int* flag;  // [slots] 0: nothing, 1: the observation erased, 2: and the point set bad
};

__global__ __launch_bounds__(kCullBlock) void cull_kf_obs_kernel(CullKfObsArgs a) {
    const MapDev& d = a.d;
    const CullDev& cu = a.c;
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * kCullWaves + (threadIdx.x >> 6);
    const int n = d.kf_mp_n[a.kf];
    if (i >= n) return;
    const long long koff = d.kf_mp_off[a.kf];
    const int mp = d.kf_mp[koff + i];
    const bool held = mp >= 0 && mp < d.n_mp;
    if (a.mode == kCullMark) {
        if (held && lane == 0) atomicMin(&cu.mark[mp], i);
        return;
    }
    int fl = 0;
    if (a.mode == kCullApply) {
        if (d.ctl[kCtlCallErr]) return;
        fl = a.flag[i];
        if (!fl) return;
    } else if (!held || cull_ld(&cu.mark[mp]) != i) {
        if (lane == 0) a.flag[i] = 0;
        return;
    }
    const long long oo = d.mp_obs_off[mp];
    const int no = d.mp_obs_n[mp];
    int p = -1;  // where this keyframe stands in the row
    for (int c = 0; c < no && p < 0; c += 64) {
        const int j = c + lane;
        const unsigned long long b = __ballot(j < no && d.mp_obs[oo + j] == a.kf);
        if (b) p = c + __ffsll((long long)b) - 1;
    }
    if (p < 0) {  // a point that does not list this keyframe is untouched (MapPoint.cc:357)
        if (a.mode == kCullCheck && lane == 0) a.flag[i] = 0;
        return;
    }
    const int ix = d.mp_idx[oo + p];
    const int by = ix >= 0 && ix < n && (cu.feat[koff + ix] & kCullRight) ? 2 : 1;  // MapPoint.cc:360-363
    if (a.mode == kCullCheck) {
        const bool bad = cu.nobs[mp] - by <= 2;  // :371
        if (bad) {
            bool unknown = false;
            for (int j = lane; j < no; j += 64) {
                if (j == p) continue;
                const int kfj = d.mp_obs[oo + j], x = d.mp_idx[oo + j];
                if (kfj < 0 || kfj >= d.n_kf || x < 0 || x >= d.kf_mp_n[kfj]) unknown = true;
            }
            if (__ballot(unknown) && lane == 0) atomicOr(&d.ctl[kCtlCallErr], 1);
        }
        if (lane == 0) a.flag[i] = bad ? 2 : 1;
        return;
    }
    // mpRefKF follows the erase ahead of the nObs decision (MapPoint.cc:367-368); SetBadFlag below
    // leaves it alone.  Every lane has read the column before lane 0 writes it.
    if (cu.ref_kf && cu.ref_kf[mp] == a.kf) {
        const int next = cull_first_observer(d, oo, no, p, lane);
        if (lane == 0) cu.ref_kf[mp] = next;
    }
    if (fl == 2) {  // MapPoint::SetBadFlag of what is left (:392-409)
        for (int j = lane; j < no; j += 64) {
            if (j == p) continue;
            const int kfj = d.mp_obs[oo + j], x = d.mp_idx[oo + j];
            if (kfj < 0 || kfj >= d.n_kf || x < 0 || x >= d.kf_mp_n[kfj]) continue;
            d.kf_mp[d.kf_mp_off[kfj] + x] = -1;
        }
        if (lane == 0) {
            d.mp_bad[mp] = 1;
            d.mp_obs_n[mp] = 0;
            cu.nobs[mp] -= by;
        }
        return;
    }
    // the row closes over position p: every lane loads before any lane stores
    int* const row = d.mp_obs + oo;
    int* const xrow = d.mp_idx + oo;
    for (int c = p; c < no - 1; c += 64) {
        const int j = c + lane;
        const bool in = j < no - 1;
        const int v = in ? row[j + 1] : 0, x = in ? xrow[j + 1] : 0;
        __builtin_amdgcn_wave_barrier();
        if (in) {
            row[j] = v;
            xrow[j] = x;
        }
        __builtin_amdgcn_wave_barrier();
    }
    if (lane == 0) {
        d.mp_obs_n[mp] = no - 1;
        cu.nobs[mp] -= by;
    }
}

__global__ __launch_bounds__(256) void cull_kf_unmark_kernel(MapDev d, CullDev cu, int kf) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= d.kf_mp_n[kf]) return;
    const int mp = d.kf_mp[d.kf_mp_off[kf] + i];
    if (mp >= 0 && mp < d.n_mp) cu.mark[mp] = kCullNoPos;
}

// The rest of SetBadFlag in one workgroup: what the erases did, as ordered lists; the spanning-tree
// tournament (:1201-1265) over the children's ordered lists and weight rows as the connection
// part left them; the leftover children (:1268-1274); mbBad (:1281).  The children rows
// themselves (AddChild / EraseChild) are the host's: out[] tells it the pairs.
struct CullKfFinishArgs {
    MapDev d;
    CovDev g;
    CullDev c;
    int kf, nc;
    const int* flag;
    const int* ch;      // the keyframe's children in key order
                        // cu.cand: 1: parent candidate, 2: a child that has left
    int* out;           // the pinned block's tail: kCullOut*, erased[slots], bad[slots], pairs[2 nc]
    int* res;
};

__global__ __launch_bounds__(kCullBlock) void cull_kf_finish_kernel(CullKfFinishArgs a) {
    __shared__ int tmp[kCullBlock / 64 + 1];
    __shared__ unsigned long long s_best;
    const MapDev& d = a.d;
    const CullDev& cu = a.c;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = d.kf_mp_n[a.kf];
    const long long koff = d.kf_mp_off[a.kf];
    int* const erased = a.out + kCullOutLists;
    int* const bad = erased + n;
    int* const pairs = bad + n;
    int n_erased = 0, n_bad = 0;
    for (int c = 0; c < n; c += kCullBlock) {
        const int i = c + tid;
        const int fl = i < n ? a.flag[i] : 0;
        const int mp = i < n ? d.kf_mp[koff + i] : -1;
        int total;
        const int ee = block_exclusive_scan<kCullBlock>(fl >= 1, tmp, total);
        if (fl >= 1) erased[n_erased + ee] = mp;
        n_erased += total;
        const int eb = block_exclusive_scan<kCullBlock>(fl == 2, tmp, total);
        if (fl == 2) bad[n_bad + eb] = mp;
        n_bad += total;
    }
    // ---- the tournament
    const int parent = d.kf_parent[a.kf];
    const bool has_parent = parent >= 0 && parent < d.n_kf;
    if (tid == 0 && has_parent) cu.cand[parent] = 1;  // :1203-1204
    __threadfence();
    __syncthreads();
    int np = 0;
    for (int round = 0; round < a.nc; ++round) {  // :1208
        if (tid == 0) s_best = 0;
        __syncthreads();
        for (int ci = wave; ci < a.nc; ci += kCullWaves) {  // :1216, pointer order
            const int c = a.ch[ci];
            if (c < 0 || c >= d.n_kf) continue;
            if ((cull_ld(&cu.cand[c]) & 2) || d.kf_bad[c]) continue;  // has left (:1261); :1222
            const int cap = a.g.cap[c];
            const int* const row = a.g.pool + a.g.off[c];
            const int nw = min(a.g.nw[c], cap), no = min(a.g.no[c], cap);
            for (int e = lane; e < no; e += 64) {  // :1230, the ordered list as it stands
                const int o = row[2ll * cap + e];
                if (o < 0 || o >= d.n_kf || !(cull_ld(&cu.cand[o]) & 1)) continue;  // :1238
                const int lo = cov_lower_bound_slots(row, nw, d.kf_key, d.kf_key[o]);
                const int w = lo < nw && row[lo] == o ? row[cap + lo] : 0;  // GetWeight: the weight map
                // `w > max` from -1 (:1243): the largest weight at the first (child, position)
                atomicMax(&s_best, ((unsigned long long)(w + 1) << 40) |
                                       ((unsigned long long)(0xffffff - ci) << 12) | (unsigned)(4095 - e));
            }
        }
        __syncthreads();
        const unsigned long long best = s_best;
        __syncthreads();
        if (!best) break;  // :1263
        const int ci = 0xffffff - (int)((best >> 12) & 0xffffff), e = 4095 - (int)(best & 4095);
        if (tid == 0) {
            const int c = a.ch[ci];
            const int pp = (a.g.pool + a.g.off[c])[2ll * a.g.cap[c] + e];
            pairs[2 * np] = c;  // :1259-1261
            pairs[2 * np + 1] = pp;
            d.kf_parent[c] = pp;
            cu.cand[c] = 3;
        }
        ++np;
        __threadfence();
        __syncthreads();
    }
    const int n_rounds = np;
    if (has_parent) {  // :1268-1274: bad children too
        for (int c0 = 0; c0 < a.nc; c0 += kCullBlock) {
            const int ci = c0 + tid;
            const int c = ci < a.nc ? a.ch[ci] : -1;
            const bool left = c >= 0 && c < d.n_kf && !(cull_ld(&cu.cand[c]) & 2);
            int total;
            const int ex = block_exclusive_scan<kCullBlock>(left, tmp, total);
            if (left) {
                pairs[2 * (np + ex)] = c;
                pairs[2 * (np + ex) + 1] = parent;
                d.kf_parent[c] = parent;
            }
            np += total;
        }
    }
    __syncthreads();
    for (int ci = tid; ci < a.nc; ci += kCullBlock) {
        const int c = a.ch[ci];
        if (c >= 0 && c < d.n_kf) cu.cand[c] = 0;
    }
    if (tid == 0) {
        if (has_parent) cu.cand[parent] = 0;
        d.kf_bad[a.kf] = 1;  // :1281
        a.out[kCullOutErased] = n_erased;
        a.out[kCullOutBad] = n_bad;
        a.out[kCullOutRounds] = n_rounds;
        a.out[kCullOutPairs] = np;
        a.out[kCullOutParent] = has_parent ? parent : -1;
    }
    __threadfence_system();
    __syncthreads();
    if (tid == 0) __hip_atomic_store(&a.res[kResDone], 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// One decision of KeyFrameCulling (LocalMapping.cc:643-695) per workgroup: waves stride the
// keyframe's slots, lanes a point's observers.
struct CullDecideArgs {
    MapDev d;
    CullDev c;
    int n, first_slot, mono;
    const int* list;
    int* res;   // [n] 1: nRedundantObservations > 0.9 * nMPs
};

__global__ __launch_bounds__(kCullBlock) void cull_decide_kernel(CullDecideArgs a) {
    __shared__ int s_n, s_r;
    const MapDev& d = a.d;
    const CullDev& cu = a.c;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int kf = a.list[blockIdx.x];
    if (kf == a.first_slot) {  // :643
        if (tid == 0) a.res[blockIdx.x] = 0;
        return;
    }
    if (tid == 0) s_n = s_r = 0;
    __syncthreads();
    const int n = d.kf_mp_n[kf];
    const long long koff = d.kf_mp_off[kf];
    const float th = cu.th_depth[kf];
    int n_mps = 0, n_red = 0;
    for (int i = wave; i < n; i += kCullWaves) {  // :653, as a vector
        const int mp = d.kf_mp[koff + i];
        if (mp < 0 || mp >= d.n_mp) continue;     // :656
        if (d.mp_bad[mp]) continue;               // :658
        if (!a.mono) {
            const float z = cu.depth[koff + i];
            if (z > th || z < 0) continue;        // :662
        }
        ++n_mps;                                  // :666
        if (cu.nobs[mp] <= 3) continue;            // :667
        const int level = cu.feat[koff + i] & (kCullRight - 1);
        const long long oo = d.mp_obs_off[mp];
        const int no = d.mp_obs_n[mp];
        int cnt = 0;
        bool unknown = false;
        for (int j = lane; j < no; j += 64) {     // :672: counting to a threshold, any order
            const int kfj = d.mp_obs[oo + j];
            if (kfj == kf) continue;              // :675
            const int x = d.mp_idx[oo + j];
            if (kfj < 0 || kfj >= d.n_kf || x < 0 || x >= d.kf_mp_n[kfj]) {
                unknown = true;
                continue;
            }
            const int level_j = cu.feat[d.kf_mp_off[kfj] + x] & (kCullRight - 1);
            if (level_j <= level + 1) ++cnt;      // :679
        }
        if (__ballot(unknown) && lane == 0) atomicOr(&d.ctl[kCtlCallErr], 1);
        if (wave_sum(cnt) >= 3) ++n_red;          // :686
    }
    if (lane == 0) {
        atomicAdd(&s_n, n_mps);
        atomicAdd(&s_r, n_red);
    }
    __syncthreads();
    // int > 0.9 * int in double equals 10 r > 9 n through 8,192 (tests/test_culling.py)
    if (tid == 0) a.res[blockIdx.x] = 10 * s_r > 9 * s_n ? 1 : 0;
}

}  // namespace orbfe

namespace {

bool cull_points_ok(const orbfe_map* m, int n, const int32_t* slots) {
    if (n < 0 || (n && !slots)) return false;
    for (int i = 0; i < n; ++i)
        if (!m->mp_ok(slots[i])) return false;
    return true;
}

// An observation whose feature index is not known cannot be EraseMapPointMatch'ed.
bool cull_idx_known(const orbfe_map* m, int mp) {
    for (int x : m->h_idx[mp])
        if (x < 0) return false;
    return true;
}

// MapPoint::SetBadFlag of distinct points whose indices are all known: one launch; the host rows follow.
int cull_apply_bad(orbfe_map* m, const std::vector<int>& slots) {
    if (slots.empty()) return ORBFE_OK;
    const int n = (int)slots.size();
    int st;
    int* d_slots;
    if ((st = store_stage_slots(m, n, slots.data(), d_slots))) return st;
    hipLaunchKernelGGL(cull_setbad_kernel, dim3((n + 3) / 4), dim3(256), 0, m->stream, m->dev(), n, d_slots);
    ORBFE_HIP(hipGetLastError());
    ORBFE_HIP(hipStreamSynchronize(m->stream));
    for (int p : slots) {
        m->h_obs[p].clear();
        m->h_idx[p].clear();
        m->mp_obs.len[p] = 0;
    }
    return ORBFE_OK;
}

// KeyFrame::EraseChild (KeyFrame.cc:1108-1112).
int cull_erase_child(orbfe_map* m, int parent, int child) {
    const RowTable& r = m->kf_ch;
    if (!r.length(parent)) return ORBFE_OK;
    std::vector<int> row((size_t)r.len[parent]);
    ORBFE_HIP(hipMemcpyAsync(row.data(), m->kf_ch_pool.buf.as<int>() + r.off[parent], sizeof(int) * row.size(),
                             hipMemcpyDeviceToHost, m->stream));
    ORBFE_HIP(hipStreamSynchronize(m->stream));
    const auto it = std::find(row.begin(), row.end(), child);
    if (it == row.end()) return ORBFE_OK;
    row.erase(it);
    return map_put_kf_ch(m, {{parent, 0, (int)row.size(), (int)row.size(), row.data(), nullptr}});
}

struct CullKfResult {
    std::vector<int> bad;                     // the points that went bad, in the order of their SetBadFlag
    std::vector<std::pair<int, int>> pairs;   // (child, new parent) in the order of ChangeParent
};

// KeyFrame::SetBadFlag past its two early returns (KeyFrame.cc:1188-1281).  A point that would go
// bad while one of its other observers has no index: ORBFE_ERR_ARG before anything changes.
int cull_kf_bad(orbfe_map* m, int slot, CullKfResult& out) {
    int st;
    if ((st = cull_ready(m))) return st;
    if (ref_made(m) && (st = ref_ready_mp(m))) return st;  // mpRefKF follows the erases
    if ((st = store_side_pools(m))) return st;
    if ((st = cov_ready(m))) return st;
    const int ns = m->kf_mp.len[slot];
    const int nc = m->kf_ch.length(slot);
    std::vector<int> children((size_t)nc);
    if (nc)
        ORBFE_HIP(hipMemcpyAsync(children.data(), m->kf_ch_pool.buf.as<int>() + m->kf_ch.off[slot],
                                 sizeof(int) * (size_t)nc, hipMemcpyDeviceToHost, m->stream));
    if ((st = m->flag.ensure(sizeof(int) * (size_t)std::max(ns, 1)))) return st;
    if ((st = store_pin_reserve(m, (size_t)kCullOutLists + 2 * (size_t)ns + 2 * (size_t)nc))) return st;
    if ((st = store_clear_err(m))) return st;
    const dim3 grid((unsigned)((ns + kCullWaves - 1) / kCullWaves));
    const dim3 ugrid((unsigned)((ns + 255) / 256));
    int err = 0;
    if (ns) {
        CullKfObsArgs a{m->dev(), cull_dev(m), slot, kCullMark, m->flag.as<int>()};
        hipLaunchKernelGGL(cull_kf_obs_kernel, grid, dim3(kCullBlock), 0, m->stream, a);
        a.mode = kCullCheck;
        hipLaunchKernelGGL(cull_kf_obs_kernel, grid, dim3(kCullBlock), 0, m->stream, a);
        ORBFE_HIP(hipGetLastError());
    }
    if ((st = store_read_err(m, err))) return st;
    if (!err) err = cov_single(m, kCovOpEraseKf, slot, -1, 0) ? 2 : 0;  // :1188-1189, :1198-1199
    // the views of what follows: the connection part may have moved the graph's pool
    CullKfObsArgs a{m->dev(), cull_dev(m), slot, kCullApply, m->flag.as<int>()};
    if (err) {
        if (ns) hipLaunchKernelGGL(cull_kf_unmark_kernel, ugrid, dim3(256), 0, m->stream, a.d, a.c, slot);
        ORBFE_HIP(hipStreamSynchronize(m->stream));
        return err == 1 ? ORBFE_ERR_ARG : ORBFE_ERR_HIP;
    }
    if (ns) {
        hipLaunchKernelGGL(cull_kf_obs_kernel, grid, dim3(kCullBlock), 0, m->stream, a);  // :1191-1193
        hipLaunchKernelGGL(cull_kf_unmark_kernel, ugrid, dim3(256), 0, m->stream, a.d, a.c, slot);
    }
    int* res = m->pin;
    __atomic_store_n(&res[kResDone], -1, __ATOMIC_RELEASE);
    CullKfFinishArgs f{};
    f.d = a.d;
    f.g = cov_dev(m);
    f.c = a.c;
    f.kf = slot;
    f.nc = nc;
    f.flag = m->flag.as<int>();
    f.ch = nc ? m->kf_ch_pool.buf.as<int>() + m->kf_ch.off[slot] : nullptr;
    f.out = m->pin_dev + kResTail;
    f.res = m->pin_dev;
    hipLaunchKernelGGL(cull_kf_finish_kernel, dim3(1), dim3(kCullBlock), 0, m->stream, f);
    ORBFE_HIP(hipGetLastError());
    if ((st = wait_words(res + kResDone, 1, -1, m->stream, 20000))) return st;
    const int* rep = m->pin + kResTail;
    const int ne = rep[kCullOutErased], nb = rep[kCullOutBad], nr = rep[kCullOutRounds];
    const int np = rep[kCullOutPairs], parent = rep[kCullOutParent];
    if (ne < 0 || ne > ns || nb < 0 || nb > ne || nr < 0 || nr > np || np > nc) return ORBFE_ERR_HIP;
    const int* erased = rep + kCullOutLists;
    const int* bad = erased + ns;
    const int* pairs = bad + ns;
    // the host rows follow the device's
    for (int i = 0; i < ne; ++i) {
        const int p = erased[i];
        if (!m->mp_ok(p)) return ORBFE_ERR_HIP;
        std::vector<int>& o = m->h_obs[p];
        const auto it = std::lower_bound(o.begin(), o.end(), slot);
        if (it == o.end() || *it != slot) return ORBFE_ERR_HIP;
        const auto xi = m->h_idx[p].begin() + (it - o.begin());
        if (*xi < 0) --m->n_unknown;
        m->h_idx[p].erase(xi);
        o.erase(it);
        m->mp_obs.len[p] = (int)o.size();
    }
    for (int i = 0; i < nb; ++i) {
        const int p = bad[i];
        m->h_obs[p].clear();
        m->h_idx[p].clear();
        m->mp_obs.len[p] = 0;
        out.bad.push_back(p);
    }
    // AddChild of every ChangeParent (:1118), this keyframe's mspChildrens without the children
    // that left (:1261; not cleared otherwise), EraseChild on the parent (:1277)
    std::vector<int> who((size_t)np), whom((size_t)np);
    for (int i = 0; i < np; ++i) {
        who[i] = pairs[2 * i];
        whom[i] = pairs[2 * i + 1];
        out.pairs.push_back({who[i], whom[i]});
    }
    if ((st = cov_add_children(m, np, who.data(), whom.data()))) return st;
    if (nr) {
        std::vector<int> left;
        for (int ch : children)
            if (std::find(who.begin(), who.begin() + nr, ch) == who.begin() + nr) left.push_back(ch);
        if ((st = map_put_kf_ch(m, {{slot, 0, (int)left.size(), (int)left.size(), left.data(), nullptr}}))) return st;
    }
    if (parent >= 0 && (st = cull_erase_child(m, parent, slot))) return st;
    return ORBFE_OK;
}

// What a SetBadFlag reports, copied out; counts beyond a capacity: ORBFE_ERR_CAPACITY.
int cull_report(const CullKfResult& r, int32_t* bad_points, int bad_cap, int32_t* n_bad, int32_t* pairs,
                int pair_cap, int32_t* n_pairs) {
    if (n_bad) *n_bad = (int)r.bad.size();
    if (n_pairs) *n_pairs = (int)r.pairs.size();
    int st = ORBFE_OK;
    if (bad_points) {
        if ((int)r.bad.size() > bad_cap) st = ORBFE_ERR_CAPACITY;
        else std::copy(r.bad.begin(), r.bad.end(), bad_points);
    }
    if (pairs) {
        if ((int)r.pairs.size() > pair_cap) st = ORBFE_ERR_CAPACITY;
        else
            for (size_t i = 0; i < r.pairs.size(); ++i) {
                pairs[2 * i] = r.pairs[i].first;
                pairs[2 * i + 1] = r.pairs[i].second;
            }
    }
    return st;
}

// KeyFrame::SetBadFlag from its top (:1174-1186).
int cull_kf_set_bad(orbfe_map* m, int slot, bool is_first, int& what, CullKfResult& r) {
    what = ORBFE_MAP_BAD_NOTHING;
    if (is_first) return ORBFE_OK;     // :1179
    if (m->h_not_erase[slot]) {        // :1181-1185
        m->h_to_erase[slot] = 1;
        what = ORBFE_MAP_BAD_DEFERRED;
        return ORBFE_OK;
    }
    const int st = cull_kf_bad(m, slot, r);
    if (st == ORBFE_OK) what = ORBFE_MAP_BAD_DONE;
    return st;
}

bool cull_report_args_ok(const int32_t* bad_points, int bad_cap, const int32_t* pairs, int pair_cap) {
    return bad_cap >= 0 && pair_cap >= 0 && (!bad_cap || bad_points) && (!pair_cap || pairs);
}

}  // namespace

extern "C" {

int orbfe_map_set_not_erase(orbfe_map* m, int slot, int flag) {
    if (!m || !m->kf_ok(slot)) return ORBFE_ERR_ARG;
    return map_guarded(m, [&]() {
        int st;
        if ((st = cull_ready(m))) return st;
        m->h_not_erase[slot] = flag ? 1 : 0;
        return (int)ORBFE_OK;
    });
}

int orbfe_map_get_erase_flags(orbfe_map* m, int slot, int32_t* not_erase, int32_t* to_be_erased) {
    if (!m || !m->kf_ok(slot)) return ORBFE_ERR_ARG;
    return map_guarded(m, [&]() {
        int st;
        if ((st = cull_ready(m))) return st;
        if (not_erase) *not_erase = m->h_not_erase[slot];
        if (to_be_erased) *to_be_erased = m->h_to_erase[slot];
        return (int)ORBFE_OK;
    });
}

int orbfe_map_set_keyframe_bad_flag(orbfe_map* m, int slot, int is_first, int32_t* what, int32_t* bad_points,
                                    int bad_cap, int32_t* n_bad, int32_t* pairs, int pair_cap, int32_t* n_pairs) {
    if (!m || !m->kf_ok(slot) || !cull_report_args_ok(bad_points, bad_cap, pairs, pair_cap)) return ORBFE_ERR_ARG;
    return map_guarded(m, [&]() {
        int st, w = ORBFE_MAP_BAD_NOTHING;
        CullKfResult r;
        if ((st = cull_ready(m))) return st;
        st = cull_kf_set_bad(m, slot, is_first != 0, w, r);
        if (what) *what = w;
        if (st) return st;
        return cull_report(r, bad_points, bad_cap, n_bad, pairs, pair_cap, n_pairs);
    });
}

int orbfe_map_set_erase(orbfe_map* m, int slot, int has_loop_edges, int is_first, int32_t* what,
                        int32_t* bad_points, int bad_cap, int32_t* n_bad, int32_t* pairs, int pair_cap,
                        int32_t* n_pairs) {
    if (!m || !m->kf_ok(slot) || !cull_report_args_ok(bad_points, bad_cap, pairs, pair_cap)) return ORBFE_ERR_ARG;
    return map_guarded(m, [&]() {
        int st, w = ORBFE_MAP_BAD_NOTHING;
        CullKfResult r;
        if ((st = cull_ready(m))) return st;
        const uint8_t was = m->h_not_erase[slot];
        if (!has_loop_edges) m->h_not_erase[slot] = 0;  // KeyFrame.cc:1162-1165
        if (m->h_to_erase[slot]) st = cull_kf_set_bad(m, slot, is_first != 0, w, r);  // :1168-1171
        if (what) *what = w;
        if (st) {
            m->h_not_erase[slot] = was;  // refused: nothing has changed
            return st;
        }
        return cull_report(r, bad_points, bad_cap, n_bad, pairs, pair_cap, n_pairs);
    });
}

int orbfe_map_cull_keyframes(orbfe_map* m, int current_slot, int n, const int32_t* kf_slots, int first_kf_slot,
                             int monocular, int32_t* result, int result_cap, int32_t* n_listed,
                             int32_t* bad_points, int bad_cap, int32_t* n_bad, int32_t* pairs, int pair_cap,
                             int32_t* n_pairs) {
    if (!m || !n_listed || result_cap < 0 || (result_cap && !result) ||
        !cull_report_args_ok(bad_points, bad_cap, pairs, pair_cap))
        return ORBFE_ERR_ARG;
    if (kf_slots ? n < 0 : !m->kf_ok(current_slot)) return ORBFE_ERR_ARG;
    if (kf_slots)
        for (int i = 0; i < n; ++i)
            if (!m->kf_ok(kf_slots[i])) return ORBFE_ERR_ARG;
    return map_guarded(m, [&]() {
        int st;
        if ((st = cull_ready(m))) return st;
        if ((st = store_side_pools(m))) return st;
        if ((st = cov_ready(m))) return st;
        // vpLocalKeyFrames (LocalMapping.cc:638): a copy, taken before anything is culled
        std::vector<int> list;
        if (kf_slots) list.assign(kf_slots, kf_slots + n);
        else {
            list.resize((size_t)m->h_no[current_slot]);
            if (!list.empty()) {
                ORBFE_HIP(hipMemcpyAsync(list.data(), m->cov_pool.buf.as<int>() + m->cov.off[current_slot] + 2ll * m->cov.cap[current_slot],
                                         sizeof(int) * list.size(), hipMemcpyDeviceToHost, m->stream));
                ORBFE_HIP(hipStreamSynchronize(m->stream));
            }
        }
        const int nl = (int)list.size();
        *n_listed = nl;
        if (nl > kCullMaxList || nl > result_cap) return (int)ORBFE_ERR_CAPACITY;
        if (m->n_unknown) return (int)ORBFE_ERR_ARG;  // an observer's octave could not be read
        if (!nl) return cull_report(CullKfResult(), bad_points, bad_cap, n_bad, pairs, pair_cap, n_pairs);
        if ((st = m->list.ensure(sizeof(int) * (size_t)nl))) return st;
        if ((st = m->decided.ensure(sizeof(int) * (size_t)nl))) return st;
        ORBFE_HIP(hipMemcpyAsync(m->list.p, list.data(), sizeof(int) * (size_t)nl, hipMemcpyHostToDevice, m->stream));
        CullKfResult r;
        std::vector<int> dec((size_t)nl);
        bool changed = false;
        for (int from = 0; from < nl;) {
            // every keyframe not yet passed decides on the map as it stands; the first that culls is
            // certain, the ones after it decide again once it is gone
            CullDecideArgs a{};
            a.d = m->dev();
            a.c = cull_dev(m);
            a.n = nl - from;
            a.first_slot = first_kf_slot;
            a.mono = monocular ? 1 : 0;
            a.list = m->list.as<int>() + from;
            a.res = m->decided.as<int>();
            int err = 0;
            if ((st = store_clear_err(m))) return st;
            hipLaunchKernelGGL(cull_decide_kernel, dim3((unsigned)a.n), dim3(kCullBlock), 0, m->stream, a);
            ORBFE_HIP(hipGetLastError());
            ORBFE_HIP(hipMemcpyAsync(dec.data(), a.res, sizeof(int) * (size_t)a.n, hipMemcpyDeviceToHost, m->stream));
            if ((st = store_read_err(m, err))) return st;
            if (err) return changed ? (int)ORBFE_ERR_HIP : (int)ORBFE_ERR_ARG;
            int i = from;
            for (; i < nl; ++i) {
                if (!dec[i - from]) {
                    result[i] = ORBFE_MAP_CULL_KEPT;
                    continue;
                }
                int what;
                if ((st = cull_kf_set_bad(m, list[i], false, what, r))) return st;  // :696
                result[i] = what == ORBFE_MAP_BAD_DONE ? ORBFE_MAP_CULL_CULLED : ORBFE_MAP_CULL_DEFERRED;
                if (what == ORBFE_MAP_BAD_DONE) {
                    changed = true;
                    break;
                }
            }
            from = i + 1;
        }
        return cull_report(r, bad_points, bad_cap, n_bad, pairs, pair_cap, n_pairs);
    });
}

int orbfe_map_set_keyframe_features(orbfe_map* m, int slot, int n, const int32_t* octaves,
                                    const float* mvu_right, const float* depth, float th_depth) {
    if (!m || !m->kf_ok(slot) || n != m->kf_mp.len[slot]) return ORBFE_ERR_ARG;
    if (octaves)
        for (int i = 0; i < n; ++i)
            if (octaves[i] < 0 || octaves[i] >= kCullRight) return ORBFE_ERR_ARG;
    return map_guarded(m, [&]() {
        int st;
        if ((st = cull_ready(m))) return st;
        if ((st = store_side_pools(m))) return st;
        std::vector<uint8_t> f((size_t)n);
        std::vector<float> d((size_t)n);
        for (int i = 0; i < n; ++i) {
            f[i] = (uint8_t)((octaves ? octaves[i] : 0) | (mvu_right && mvu_right[i] >= 0 ? kCullRight : 0));
            d[i] = depth ? depth[i] : -1.f;
        }
        if (n) {
            const long long off = m->kf_mp.off[slot];
            ORBFE_HIP(hipMemcpyAsync(m->feat_pool.buf.as<uint8_t>() + off, f.data(), (size_t)n, hipMemcpyHostToDevice, m->stream));
            ORBFE_HIP(hipMemcpyAsync(m->depth_pool.buf.as<float>() + off, d.data(), sizeof(float) * (size_t)n,
                                     hipMemcpyHostToDevice, m->stream));
        }
        ORBFE_HIP(hipMemcpyAsync(m->at<float>(kColThDepth) + slot, &th_depth, sizeof(float), hipMemcpyHostToDevice, m->stream));
        ORBFE_HIP(hipStreamSynchronize(m->stream));
        m->h_feat[slot] = std::move(f);
        m->h_th_depth[slot] = th_depth;
        return (int)ORBFE_OK;
    });
}

int orbfe_map_get_keyframe_features(orbfe_map* m, int slot, int cap, int32_t* octaves, uint8_t* has_right,
                                    float* depth, float* th_depth, int32_t* n) {
    if (!m || !n || cap < 0 || !m->kf_ok(slot)) return ORBFE_ERR_ARG;
    return map_guarded(m, [&]() {
        int st;
        if ((st = cull_ready(m))) return st;
        if ((st = store_side_pools(m))) return st;
        *n = m->kf_mp.len[slot];
        if (th_depth) *th_depth = m->h_th_depth[slot];
        if (*n > cap) return (int)ORBFE_ERR_CAPACITY;
        if (!*n) return (int)ORBFE_OK;
        std::vector<uint8_t> f((size_t)*n);
        const long long off = m->kf_mp.off[slot];
        ORBFE_HIP(hipMemcpyAsync(f.data(), m->feat_pool.buf.as<uint8_t>() + off, (size_t)*n, hipMemcpyDeviceToHost, m->stream));
        if (depth)
            ORBFE_HIP(hipMemcpyAsync(depth, m->depth_pool.buf.as<float>() + off, sizeof(float) * (size_t)*n,
                                     hipMemcpyDeviceToHost, m->stream));
        ORBFE_HIP(hipStreamSynchronize(m->stream));
        for (int i = 0; i < *n; ++i) {
            if (octaves) octaves[i] = f[i] & (kCullRight - 1);
            if (has_right) has_right[i] = f[i] & kCullRight ? 1 : 0;
        }
        return (int)ORBFE_OK;
    });
}

int orbfe_map_set_point_counters(orbfe_map* m, int n, const int32_t* mp_slots, const int32_t* n_obs,
                                 const int32_t* found, const int32_t* visible, const int64_t* first_kf_id) {
    if (!m || !cull_points_ok(m, n, mp_slots)) return ORBFE_ERR_ARG;
    return map_guarded(m, [&]() {
        int st;
        if ((st = cull_ready(m))) return st;
        if (n_obs && (st = store_set<int>(m, m->at<int>(kColNobs), n, mp_slots, n_obs))) return st;
        if (found && (st = store_set<int>(m, m->at<int>(kColFound), n, mp_slots, found))) return st;
        if (visible && (st = store_set<int>(m, m->at<int>(kColVisible), n, mp_slots, visible))) return st;
        if (first_kf_id && (st = store_set<long long>(m, m->at<long long>(kColFirstKf), n, mp_slots,
                                                      reinterpret_cast<const long long*>(first_kf_id))))
            return st;
        return (int)ORBFE_OK;
    });
}

int orbfe_map_get_point_counters(orbfe_map* m, int n, const int32_t* mp_slots, int32_t* n_obs, int32_t* found,
                                 int32_t* visible, int64_t* first_kf_id) {
    if (!m || !cull_points_ok(m, n, mp_slots)) return ORBFE_ERR_ARG;
    return map_guarded(m, [&]() {
        int st;
        if ((st = cull_ready(m))) return st;
        if (n_obs && (st = store_get<int>(m, m->at<int>(kColNobs), n, mp_slots, n_obs))) return st;
        if (found && (st = store_get<int>(m, m->at<int>(kColFound), n, mp_slots, found))) return st;
        if (visible && (st = store_get<int>(m, m->at<int>(kColVisible), n, mp_slots, visible))) return st;
        if (first_kf_id && (st = store_get<long long>(m, m->at<long long>(kColFirstKf), n, mp_slots,
                                                      reinterpret_cast<long long*>(first_kf_id))))
            return st;
        return (int)ORBFE_OK;
    });
}

int orbfe_map_increase_counters(orbfe_map* m, int kind, int n, const int32_t* mp_slots, const int32_t* amounts) {
    if (!m || (kind != ORBFE_MAP_FOUND && kind != ORBFE_MAP_VISIBLE) || !cull_points_ok(m, n, mp_slots))
        return ORBFE_ERR_ARG;
    return map_guarded(m, [&]() {
        int st;
        if ((st = cull_ready(m))) return st;
        return store_add(m, m->at<int>(kind == ORBFE_MAP_FOUND ? kColFound : kColVisible), n, mp_slots, amounts, 1);
    });
}

int orbfe_map_increase_counters_device(orbfe_map* m, int kind, int n, const int32_t* d_mp_slots,
                                       const uint8_t* d_mask) {
    if (!m || (kind != ORBFE_MAP_FOUND && kind != ORBFE_MAP_VISIBLE) || n < 0 || (n && !d_mp_slots))
        return ORBFE_ERR_ARG;
    if (!n) return ORBFE_OK;
    return map_guarded(m, [&]() {
        int st;
        if ((st = cull_ready(m))) return st;
        int* dst = m->at<int>(kind == ORBFE_MAP_FOUND ? kColFound : kColVisible);
        int err = 0;
        if ((st = store_clear_err(m))) return st;
        for (int apply = 0; apply < 2; ++apply)
            hipLaunchKernelGGL(cull_add_masked_kernel, dim3((n + 255) / 256), dim3(256), 0, m->stream, n,
                               d_mp_slots, d_mask, m->n_mp, apply, dst, m->call_err());
        ORBFE_HIP(hipGetLastError());
        if ((st = store_read_err(m, err))) return st;
        return err ? (int)ORBFE_ERR_ARG : (int)ORBFE_OK;
    });
}

int orbfe_map_set_point_bad_flag(orbfe_map* m, int n, const int32_t* mp_slots) {
    if (!m || !cull_points_ok(m, n, mp_slots)) return ORBFE_ERR_ARG;
    std::vector<int> s(mp_slots, mp_slots + n);
    std::sort(s.begin(), s.end());
    s.erase(std::unique(s.begin(), s.end()), s.end());
    for (int p : s)
        if (!cull_idx_known(m, p)) return ORBFE_ERR_ARG;
    return map_guarded(m, [&]() {
        int st;
        if ((st = cull_ready(m))) return st;
        return cull_apply_bad(m, s);
    });
}

int orbfe_map_erase_observation(orbfe_map* m, int mp_slot, int kf_slot, int32_t* went_bad) {
    if (!m || !m->mp_ok(mp_slot) || !m->kf_ok(kf_slot)) return ORBFE_ERR_ARG;
    if (went_bad) *went_bad = 0;
    const std::vector<int>& o = m->h_obs[mp_slot];
    const auto it = std::lower_bound(o.begin(), o.end(), kf_slot);
    if (it == o.end() || *it != kf_slot) return ORBFE_OK;  // MapPoint.cc:357
    return map_guarded(m, [&]() {
        int st;
        if ((st = cull_ready(m))) return st;
        const int ix = m->h_idx[mp_slot][it - o.begin()];
        const int by = ix >= 0 && map_has_right(m, kf_slot, ix) ? 2 : 1;  // :360-363
        int32_t nobs = 0, s = mp_slot, k = kf_slot;
        if ((st = store_get<int>(m, m->at<int>(kColNobs), 1, &s, &nobs))) return st;
        const bool bad = nobs - by <= 2;  // :371
        if (bad)
            for (size_t j = 0; j < o.size(); ++j)
                if (o[j] != kf_slot && m->h_idx[mp_slot][j] < 0) return (int)ORBFE_ERR_ARG;
        if ((st = orbfe_map_erase_observations(m, 1, &s, &k))) return st;
        if (bad && (st = cull_apply_bad(m, {mp_slot}))) return st;  // :377
        if (went_bad) *went_bad = bad ? 1 : 0;
        return (int)ORBFE_OK;
    });
}

int orbfe_map_cull_points(orbfe_map* m, int64_t current_kf_id, int monocular, int32_t* list, int n_in,
                          int32_t* n_out, int32_t* culled, int32_t* n_culled) {
    if (!m || !n_out || !n_culled || !cull_points_ok(m, n_in, list) || (n_in && !culled) ||
        current_kf_id < 0 || current_kf_id > 0x7fffffffll)
        return ORBFE_ERR_ARG;
    *n_out = *n_culled = 0;
    if (!n_in) return ORBFE_OK;
    return map_guarded(m, [&]() {
        int st;
        if ((st = cull_ready(m))) return st;
        if ((st = store_pin_reserve(m, 2 * (size_t)n_in))) return st;
        int* d_list;
        if ((st = store_stage_slots(m, n_in, list, d_list))) return st;
        int* res = m->pin;
        res[kResCullStatus] = ORBFE_OK;
        __atomic_store_n(&res[kResDone], -1, __ATOMIC_RELEASE);
        CullPointsArgs a{};
        a.d = m->dev();
        a.c = cull_dev(m);
        a.n = n_in;
        a.th_obs = monocular ? 2 : 3;  // LocalMapping.cc:176-181
        a.cur = (int)current_kf_id;
        a.list = d_list;
        a.kept = m->pin_dev + kResTail;
        a.culled = m->pin_dev + kResTail + n_in;
        a.res = m->pin_dev;
        hipLaunchKernelGGL(cull_points_kernel, dim3(1), dim3(kCullBlock), 0, m->stream, a);
        ORBFE_HIP(hipGetLastError());
        if ((st = wait_words(res + kResDone, 1, -1, m->stream, 20000))) return st;
        if (res[kResCullStatus] != ORBFE_OK) return res[kResCullStatus];
        const int nk = res[kResKept], nc = res[kResCulled];
        if (nk < 0 || nc < 0 || nk + nc > n_in) return (int)ORBFE_ERR_HIP;
        const int* kept = m->pin + kResTail;
        const std::vector<int> gone(kept + n_in, kept + n_in + nc);
        for (int p : gone)
            if (!m->mp_ok(p) || !cull_idx_known(m, p)) return (int)ORBFE_ERR_ARG;
        if ((st = cull_apply_bad(m, gone))) return st;
        std::copy(kept, kept + nk, list);
        std::copy(gone.begin(), gone.end(), culled);
        *n_out = nk;
        *n_culled = nc;
        return (int)ORBFE_OK;
    });
}

int orbfe_map_tracked_map_points(orbfe_map* m, int slot, int min_obs, int32_t* n) {
    if (!m || !n || !m->kf_ok(slot)) return ORBFE_ERR_ARG;
    return map_guarded(m, [&]() {
        int st;
        if ((st = cull_ready(m))) return st;
        int* res = m->pin;
        __atomic_store_n(&res[kResDone], -1, __ATOMIC_RELEASE);
        hipLaunchKernelGGL(cull_tracked_kernel, dim3(1), dim3(kCullBlock), 0, m->stream, m->dev(), cull_dev(m),
                           slot, min_obs, m->pin_dev);
        ORBFE_HIP(hipGetLastError());
        if ((st = wait_words(res + kResDone, 1, -1, m->stream, 20000))) return st;
        *n = res[kResValue];
        return (int)ORBFE_OK;
    });
}

int orbfe_map_get_keyframe_points(orbfe_map* m, int slot, int32_t* mp_slots, int cap, int32_t* n) {
    if (!m || !n || cap < 0 || (cap && !mp_slots) || !m->kf_ok(slot)) return ORBFE_ERR_ARG;
    *n = m->kf_mp.len[slot];
    if (*n > cap) return ORBFE_ERR_CAPACITY;
    if (!*n) return ORBFE_OK;
    return map_guarded(m, [&]() {
        ORBFE_HIP(hipMemcpyAsync(mp_slots, m->kf_mp_pool.buf.as<int>() + m->kf_mp.off[slot], sizeof(int) * (size_t)*n,
                                 hipMemcpyDeviceToHost, m->stream));
        ORBFE_HIP(hipStreamSynchronize(m->stream));
        return (int)ORBFE_OK;
    });
}

int orbfe_map_get_observations(orbfe_map* m, int mp_slot, int32_t* kf_slots, int32_t* idx, int cap, int32_t* n) {
    if (!m || !n || cap < 0 || (cap && !kf_slots) || !m->mp_ok(mp_slot)) return ORBFE_ERR_ARG;
    return map_guarded(m, [&]() {
        int len = 0;
        ORBFE_HIP(hipMemcpyAsync(&len, m->at<int>(kColMpObsLen) + mp_slot, sizeof(int), hipMemcpyDeviceToHost, m->stream));
        ORBFE_HIP(hipStreamSynchronize(m->stream));
        const std::vector<int>& o = m->h_obs[mp_slot];
        if (len != (int)o.size()) return (int)ORBFE_ERR_HIP;  // the host rows are the device's
        *n = len;
        if (*n > cap) return (int)ORBFE_ERR_CAPACITY;
        if (!*n) return (int)ORBFE_OK;
        std::vector<int> x((size_t)*n);
        const long long off = m->mp_obs.off[mp_slot];
        ORBFE_HIP(hipMemcpyAsync(kf_slots, m->mp_obs_pool.buf.as<int>() + off, sizeof(int) * (size_t)*n,
                                 hipMemcpyDeviceToHost, m->stream));
        ORBFE_HIP(hipMemcpyAsync(x.data(), m->mp_idx_pool.buf.as<int>() + off, sizeof(int) * (size_t)*n,
                                 hipMemcpyDeviceToHost, m->stream));
        ORBFE_HIP(hipStreamSynchronize(m->stream));
        if (!std::equal(o.begin(), o.end(), kf_slots) || x != m->h_idx[mp_slot]) return (int)ORBFE_ERR_HIP;
        if (idx) std::copy(x.begin(), x.end(), idx);
        return (int)ORBFE_OK;
    });
}

int orbfe_map_get_bad_flags(orbfe_map* m, int kind, int n, const int32_t* slots, uint8_t* bad) {
    if (!m || (kind != ORBFE_MAP_KEYFRAMES && kind != ORBFE_MAP_POINTS) || n < 0 || (n && (!slots || !bad)))
        return ORBFE_ERR_ARG;
    for (int i = 0; i < n; ++i)
        if (kind == ORBFE_MAP_KEYFRAMES ? !m->kf_ok(slots[i]) : !m->mp_ok(slots[i])) return ORBFE_ERR_ARG;
    return map_guarded(m, [&]() {
        int st;
        if ((st = cull_ready(m))) return st;
        return store_get<uint8_t>(m, m->at<uint8_t>(kind == ORBFE_MAP_KEYFRAMES ? kColKfBad : kColMpBad), n, slots, bad);
    });
}

}  // extern "C"
