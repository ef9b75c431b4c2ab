// orbfe_map_store.hip — the store under the device map: the orbfe_map handle, the columns of its
// keyframes and points, its ragged row tables and their side pools, staging, the control and the
// pinned block, and the scatter / gather / add helpers of the mutators ("The map's
// store").  orbfe_localmap.hip, orbfe_covis.hip, orbfe_cull.hip and orbfe_refresh.hip hold their
// kernels, argument structs and entry points on top of it; the arithmetic is in orbfe_map_plan.hpp.
//
// Columns.  kMapColumns gives every per-keyframe and per-point array its group, element size,
// default and whether its contents survive growth.  A buffer is filled with its default when it
// is allocated and its live prefix is refilled on clear, so an element nobody has written since
// reads its default and covering more elements (store_cover) is bookkeeping.  The core groups
// are made with the handle; the covis and cull groups by their first call, covering the map as it
// then is.  store_grow is the one routine that reallocates a group.
//
// Row tables.  kf_mp, kf_ch and mp_obs are rows of ints written whole (map_rows_kernel); cov is
// the covisibility graph, rows of four arrays that keep their contents on a move
// (cov_move_kernel, orbfe_covis.hip).  A side pool shares a table's offsets and grows with it:
//   mp_idx       the feature indices beside mp_obs.  Every writer writes both at equal lengths:
//                map_change_observations puts the two rows in one store_put_rows; cull_apply_bad
//                and cull_kf_bad's host follow-up shorten or clear both host rows together;
//                cull_setbad_kernel and cull_kf_obs_kernel close or clear both device rows under
//                the one length; orbfe_map_add_points starts both empty.  So one offset column
//                and one length column serve both.
//   feat, depth  per keypoint beside kf_mp (whose rows never move: only orbfe_map_add_keyframe
//                sets a length), made by the first call that reads or writes them.
//   kdesc        the keypoints' descriptor rows, 32 bytes each, beside kf_mp as well; made by the
//                first call of orbfe_refresh.hip that needs it (store_desc_pool), so a handle that
//                never refreshes a point holds none.
//
// What may move when: a column group in store_grow, a pool in store_put_rows / cov_reserve /
// store_side_pools, a staging buffer in store_borrow, the pinned block in store_pin_reserve; all
// of them between launches only, and every device view (MapDev, CovDev, CullDev) is built after
// the last of them, immediately before the launches that use it.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <new>
#include <unordered_map>
#include <vector>

#include "../../include/orbfe.h"
#include "orbfe_device.hpp"
#include "orbfe_map_plan.hpp"

namespace orbfe {

constexpr int kMapBlock = 1024;
constexpr int kMapMaxVoted = ORBFE_MAP_MAX_VOTED;        // keyframes map_local_kf_kernel sorts in LDS
constexpr int kMapListCap = kMapMaxVoted + 8;            // phase 2 adds at most 3 to a list of <= 80
constexpr int kMapMaxSlots = ORBFE_MAP_MAX_KF_SLOTS;     // mvpMapPoints of one keyframe; the pitch of a position
constexpr int kMapNeigh = 10;                            // GetBestCovisibilityKeyFrames(10)
constexpr int kMapChunks = kMapMaxSlots / kMapBlock;
constexpr int kCullRight = 0x80;                         // the feature byte: octave | kCullRight

// device control words (ints).  kCtlErr is the query's (map_vote_kernel raises it,
// map_local_kf_kernel reads and clears it); kCtlCallErr is the error word of every other call:
// cleared before its launches, read back after them.
enum { kCtlTouched, kCtlErr, kCtlNKf, kCtlRef, kCtlNMp, kCtlRun, kCtlStatus, kCtlCountA, kCtlCountB,
       kCtlCallErr, kCtlWords = 16 };
// the pinned block: a fixed head of result words, then a tail that holds the keyframe list of a
// query or the lists a culling call reports.  The tail starts on a page of its own, as the
// culling reports' block did: what a kernel streams into it shares no cache line, and no
// adjacent one, with the done word the host polls.
enum { kResNKf, kResRef, kResNMp, kResStatus, kResDone, kResKept, kResCulled, kResCullStatus, kResValue,
       kResTail = 1024 };

enum { kGroupCoreKf, kGroupCoreMp, kGroupCovis, kGroupCullMp, kGroupCullKf, kGroupRefMp, kGroupRefKf, kMapGroups };
enum {
    kColKfKey, kColKfBad, kColKfStamp, kColKfNeigh, kColKfParent, kColKfCnt, kColKfMpOff, kColKfMpLen,
    kColKfChOff, kColKfChLen,
    kColMpBad, kColMpStamp, kColMpObsOff, kColMpObsLen, kColFirstPos, kColLocalMp,
    kColCovOff, kColCovCap, kColCovNw, kColCovNo, kColCovFirst, kColCovRes, kColCovPos,
    kColNobs, kColFound, kColVisible, kColFirstKf, kColMark,
    kColThDepth, kColCand,
    kColRefKf,
    kColCenter, kColDescSet,
    kMapCols
};

// A default is a repeated byte, or (word) one 4-byte value written by store_fill_kernel.
struct MapFill {
    bool word;
    unsigned v;
};
struct MapColumn {
    int group, per;
    MapFill fill;
    bool keep;  // false: scratch that is at `fill` between calls; refilled, not copied, on growth
};
constexpr int kMapNoPos = 0x7f7f7f7f;  // first_pos / mark of a point no position has claimed
constexpr MapColumn kMapColumns[kMapCols] = {
    // a new KeyFrame: key 0 until map_kf_key_kernel, not bad, stamp 0 (KeyFrame.cc:35), no
    // neighbours, no parent, no points, no children
    {kGroupCoreKf, 8, {false, 0x00}, true},                 // kf_key
    {kGroupCoreKf, 1, {false, 0x00}, true},                 // kf_bad
    {kGroupCoreKf, 8, {false, 0x00}, true},                 // kf_stamp
    {kGroupCoreKf, 4 * kMapNeigh, {false, 0xff}, true},     // kf_neigh: -1
    {kGroupCoreKf, 4, {false, 0xff}, true},                 // kf_parent: -1
    {kGroupCoreKf, 4, {false, 0x00}, false},                // kf_cnt: all 0 between queries
    {kGroupCoreKf, 8, {false, 0x00}, true},                 // kf_mp off
    {kGroupCoreKf, 4, {false, 0x00}, true},                 // kf_mp len
    {kGroupCoreKf, 8, {false, 0x00}, true},                 // kf_ch off
    {kGroupCoreKf, 4, {false, 0x00}, true},                 // kf_ch len
    // a new MapPoint: not bad, stamp 0 (MapPoint.cc:36, :55), no observations
    {kGroupCoreMp, 1, {false, 0x00}, true},                 // mp_bad
    {kGroupCoreMp, 8, {false, 0x00}, true},                 // mp_stamp
    {kGroupCoreMp, 8, {false, 0x00}, true},                 // mp_obs off
    {kGroupCoreMp, 4, {false, 0x00}, true},                 // mp_obs len
    {kGroupCoreMp, 4, {false, 0x7f}, false},                // first_pos: all kMapNoPos between queries
    {kGroupCoreMp, 4, {false, 0x00}, true},                 // local_mp
    // the covisibility graph: no connections, mbFirstConnection set (KeyFrame.cc:41)
    {kGroupCovis, 8, {false, 0x00}, true},                  // cov off
    {kGroupCovis, 4, {false, 0x00}, true},                  // cov cap
    {kGroupCovis, 4, {false, 0x00}, true},                  // cov nw
    {kGroupCovis, 4, {false, 0x00}, true},                  // cov no
    {kGroupCovis, 1, {false, 0x01}, true},                  // cov first
    {kGroupCovis, 12, {false, 0x00}, false},                // cov res: written before it is read
    {kGroupCovis, 4, {false, 0xff}, false},                 // cov pos: set by every batch
    // the culling counters: nObs 0, mnFound = mnVisible = 1 (MapPoint.cc:37-38), mnFirstKFid 0
    {kGroupCullMp, 4, {false, 0x00}, true},                 // nobs
    {kGroupCullMp, 4, {true, 1u}, true},                    // found
    {kGroupCullMp, 4, {true, 1u}, true},                    // visible
    {kGroupCullMp, 8, {false, 0x00}, true},                 // first_kf
    {kGroupCullMp, 4, {false, 0x7f}, false},                // mark: all kMapNoPos between calls
    {kGroupCullKf, 4, {false, 0x00}, true},                 // th_depth: 0.f
    {kGroupCullKf, 4, {false, 0x00}, false},                // cand: all 0 between calls
    // what MapPoint::UpdateNormalAndDepth and ComputeDistinctiveDescriptors read (orbfe_refresh.hip):
    // mpRefKF as a keyframe slot, GetCameraCenter(), whether the keyframe's descriptors were set
    {kGroupRefMp, 4, {false, 0xff}, true},                  // ref_kf: -1
    {kGroupRefKf, 12, {false, 0x00}, true},                 // center: (0, 0, 0)
    {kGroupRefKf, 1, {false, 0x00}, true},                  // desc_set
};
// what no orbfe_map_set_keyframe_features wrote: octave 0 and no right coordinate; depth -1.f
constexpr MapFill kFillZero = {false, 0x00};
constexpr MapFill kFillFeat = {false, 0x00};
constexpr MapFill kFillDepth = {true, 0xbf800000u};
constexpr int kMapDescBytes = 32;                         // one row of mDescriptors
constexpr int kMapMaxLevels = 128;                        // mvScaleFactors of a map

// ---- the device views, one per group: built by orbfe_map::dev(), cov_dev() and cull_dev()

struct MapDev {
    int n_kf, n_mp;
    const unsigned long long* kf_key;
    uint8_t* kf_bad;
    unsigned long long* kf_stamp;
    const long long* kf_mp_off;
    const int* kf_mp_n;
    int* kf_mp;
    int* kf_neigh;
    const long long* kf_ch_off;
    const int* kf_ch_n;
    const int* kf_ch;
    int* kf_parent;
    uint8_t* mp_bad;
    unsigned long long* mp_stamp;
    const long long* mp_obs_off;
    int* mp_obs_n;
    int* mp_obs;
    int* mp_idx;  // at mp_obs' offsets, of mp_obs' lengths
    // scratch: kf_cnt is all 0 and first_pos all kMapNoPos between queries
    int* kf_cnt;
    int* touched;
    int* first_pos;
    int* ctl;
    int* local_kf;
    int* local_mp;
    int* blk;
};

// The covisibility graph: row j is 4 arrays of cap[j] ints at pool + off[j].
struct CovDev {
    int* pool;
    long long* off;
    int* cap;
    int* nw;
    int* no;
    uint8_t* first;
    int* res;  // [3 n_kf] deciding: the weight map's and the list's new length, act
    int* pos;  // [n_kf] position in the batch or -1
};

struct CullDev {
    int* nobs;
    int* found;
    int* visible;
    const long long* first_kf;
    int* mark;             // all kMapNoPos between calls
    const uint8_t* feat;   // octave | kCullRight, at the offsets of kf_mp's pool
    const float* depth;
    const float* th_depth; // [n_kf]
    int* cand;             // [n_kf] all 0 between calls
    int* ref_kf;           // [n_mp] mpRefKF, or NULL while nobody has made the column
};

__global__ __launch_bounds__(256) void store_fill_kernel(long long n, unsigned* dst, unsigned v) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) dst[i] = v;
}

// dst[slots[i]] = vals ? vals[i] : value
template <class T>
__global__ __launch_bounds__(256) void store_set_kernel(int n, const int* slots, const T* vals, T value,
                                                        T* dst) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) dst[slots[i]] = vals ? vals[i] : value;
}

template <class T>
__global__ __launch_bounds__(256) void store_get_kernel(int n, const int* slots, const T* src, T* out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = src[slots[i]];
}

// dst[slots[i]] += amounts ? amounts[i] : amount; a repeated slot adds up.
__global__ __launch_bounds__(256) void store_add_kernel(int n, const int* slots, const int* amounts,
                                                        int amount, int* dst) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) atomicAdd(&dst[slots[i]], amounts ? amounts[i] : amount);
}

// One row write of a ragged table: n ints from staged[src ..) to pool[dst ..), the same from
// staged2 into the side pool when there is one, and the row's (offset, length) when row >= 0.
// One wave per item.
struct MapRowItem {
    long long dst, new_off;
    int src, n, row, new_n;
};

__global__ __launch_bounds__(256) void map_rows_kernel(int n_items, const MapRowItem* items,
                                                       const int* staged, int* pool, const int* staged2,
                                                       int* pool2, long long* off, int* len) {
    const int w = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= n_items) return;
    const MapRowItem it = items[w];
    const int lane = threadIdx.x & 63;
    for (int j = lane; j < it.n; j += 64) pool[it.dst + j] = staged[it.src + j];
    if (pool2)
        for (int j = lane; j < it.n; j += 64) pool2[it.dst + j] = staged2[it.src + j];
    if (lane == 0 && it.row >= 0) {
        off[it.row] = it.new_off;
        len[it.row] = it.new_n;
    }
}

}  // namespace orbfe

using namespace orbfe;

namespace {

// A pool of a row table, or one at a table's offsets.
struct MapPool {
    DevBuf buf;
    long long alloc = 0;  // elements
};

enum { kStageSlots, kStageVals, kStageItems, kStageOut, kStageRoles };

struct MapRowWrite {
    int row, first, n;   // n ints at offset `first` of the row
    int new_len;         // the row's length afterwards, or -1: unchanged
    const int* data;
    const int* data2;    // the side pool's, when the table is written with one
};

}  // namespace

struct orbfe_map {
    int device = 0;
    int n_kf = 0, n_mp = 0;
    int max_slots = 0;  // the longest mvpMapPoints: the point kernels' grid
    std::unordered_map<uint64_t, int> by_key;
    std::vector<uint64_t> h_key;
    std::vector<std::vector<int>> h_obs;  // sorted
    std::vector<std::vector<int>> h_idx;  // mObservations[pKF] of h_obs' entries, or -1
    long long n_unknown = 0;              // entries of h_idx that are -1
    std::vector<int> h_local;             // the list as of the last query / set_local_keyframes
    int h_ref = -1, h_n_local_mp = 0;
    // the covisibility graph's lengths and the culling state the host keeps
    std::vector<int> h_nw, h_no;
    std::vector<std::vector<uint8_t>> h_feat;  // per keyframe; empty: never set
    std::vector<float> h_th_depth;
    std::vector<uint8_t> h_not_erase, h_to_erase;  // mbNotErase, mbToBeErased

    ColumnGroup group[kMapGroups];
    DevBuf col[kMapCols];
    RowTable kf_mp{1, 4, 4096}, kf_ch{1, 4, 4096}, mp_obs{1, 4, 4096}, cov{4, 8, 1 << 16};
    MapPool kf_mp_pool, kf_ch_pool, mp_obs_pool, cov_pool;
    MapPool mp_idx_pool;            // side pool of mp_obs
    MapPool feat_pool, depth_pool;  // side pools of kf_mp
    MapPool kdesc_pool;             // side pool of kf_mp: kMapDescBytes per keypoint
    DevBuf scale;                   // mvScaleFactors: kMapMaxLevels floats, made by its setter
    std::vector<float> h_scale;     // the same; empty: never set
    std::vector<uint8_t> h_desc_set;  // per keyframe: orbfe_map_set_keyframe_descriptors has run
    DevBuf touched, ctl, local_kf, blk;  // the query's fixed scratch
    DevBuf stage[kStageRoles];
    // scratch that lives across a call's nested mutators: the counters of an UpdateConnections
    // batch; the flags, the list and the decisions of a keyframe culling
    DevBuf batch, allow, c_n, c_off, c_slot, c_w, pout, flag, list, decided;
    hipStream_t own = nullptr, stream = nullptr;
    int* pin = nullptr;
    int* pin_dev = nullptr;
    size_t pin_tail = 0;  // ints after the head

    template <class T> T* at(int c) const { return col[c].as<T>(); }
    int* call_err() const { return ctl.as<int>() + kCtlCallErr; }

    MapDev dev() const {
        MapDev d;
        d.n_kf = n_kf;
        d.n_mp = n_mp;
        d.kf_key = at<unsigned long long>(kColKfKey);
        d.kf_bad = at<uint8_t>(kColKfBad);
        d.kf_stamp = at<unsigned long long>(kColKfStamp);
        d.kf_mp_off = at<long long>(kColKfMpOff);
        d.kf_mp_n = at<int>(kColKfMpLen);
        d.kf_mp = kf_mp_pool.buf.as<int>();
        d.kf_neigh = at<int>(kColKfNeigh);
        d.kf_ch_off = at<long long>(kColKfChOff);
        d.kf_ch_n = at<int>(kColKfChLen);
        d.kf_ch = kf_ch_pool.buf.as<int>();
        d.kf_parent = at<int>(kColKfParent);
        d.mp_bad = at<uint8_t>(kColMpBad);
        d.mp_stamp = at<unsigned long long>(kColMpStamp);
        d.mp_obs_off = at<long long>(kColMpObsOff);
        d.mp_obs_n = at<int>(kColMpObsLen);
        d.mp_obs = mp_obs_pool.buf.as<int>();
        d.mp_idx = mp_idx_pool.buf.as<int>();
        d.kf_cnt = at<int>(kColKfCnt);
        d.touched = touched.as<int>();
        d.first_pos = at<int>(kColFirstPos);
        d.ctl = ctl.as<int>();
        d.local_kf = local_kf.as<int>();
        d.local_mp = at<int>(kColLocalMp);
        d.blk = blk.as<int>();
        return d;
    }
    bool kf_ok(int s) const { return s >= 0 && s < n_kf; }
    bool mp_ok(int s) const { return s >= 0 && s < n_mp; }
    ~orbfe_map() {
        if (pin) hipHostFree(pin);
        if (own) hipStreamDestroy(own);
    }
};

namespace {

CovDev cov_dev(const orbfe_map* m) {
    CovDev g;
    g.pool = m->cov_pool.buf.as<int>();
    g.off = m->at<long long>(kColCovOff);
    g.cap = m->at<int>(kColCovCap);
    g.nw = m->at<int>(kColCovNw);
    g.no = m->at<int>(kColCovNo);
    g.first = m->at<uint8_t>(kColCovFirst);
    g.res = m->at<int>(kColCovRes);
    g.pos = m->at<int>(kColCovPos);
    return g;
}

CullDev cull_dev(const orbfe_map* m) {
    CullDev c;
    c.nobs = m->at<int>(kColNobs);
    c.found = m->at<int>(kColFound);
    c.visible = m->at<int>(kColVisible);
    c.first_kf = m->at<long long>(kColFirstKf);
    c.mark = m->at<int>(kColMark);
    c.feat = m->feat_pool.buf.as<uint8_t>();
    c.depth = m->depth_pool.buf.as<float>();
    c.th_depth = m->at<float>(kColThDepth);
    c.cand = m->at<int>(kColCand);
    c.ref_kf = m->group[kGroupRefMp].alloc ? m->at<int>(kColRefKf) : nullptr;
    return c;
}

// Whether mvuRight[idx] of a keyframe is >= 0 as orbfe_map_set_keyframe_features left it.
bool map_has_right(const orbfe_map* m, int kf, int idx) {
    if (kf < 0 || (size_t)kf >= m->h_feat.size()) return false;
    const std::vector<uint8_t>& f = m->h_feat[kf];
    return idx >= 0 && (size_t)idx < f.size() && (f[idx] & kCullRight);
}

template <class F>
int map_guarded(orbfe_map* m, F&& f) {
    try {
        DeviceGuard dg(m->device);
        return f();
    } catch (const std::bad_alloc&) {
        return ORBFE_ERR_NOMEM;
    } catch (...) {
        return ORBFE_ERR_HIP;
    }
}

// `n` elements of `per` bytes at p set to the default `f`.
int store_fill(orbfe_map* m, void* p, size_t per, long long n, MapFill f) {
    if (n <= 0) return ORBFE_OK;
    if (!f.word) {
        ORBFE_HIP(hipMemsetAsync(p, (int)f.v, per * (size_t)n, m->stream));
        return ORBFE_OK;
    }
    hipLaunchKernelGGL(store_fill_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, m->stream, n,
                       static_cast<unsigned*>(p), f.v);
    ORBFE_HIP(hipGetLastError());
    return ORBFE_OK;
}

// `nb` made to hold n elements: all at the default, then the first `keep` of `old`.  Enqueued
// only: the caller synchronises before `old` is released.
int store_regrow(orbfe_map* m, const DevBuf& old, DevBuf& nb, size_t per, long long keep, long long n,
                 MapFill f) {
    int st;
    if ((st = nb.ensure(per * (size_t)n))) return st;
    if ((st = store_fill(m, nb.p, per, n, f))) return st;
    if (old.p && keep > 0)
        ORBFE_HIP(hipMemcpyAsync(nb.p, old.p, per * (size_t)keep, hipMemcpyDeviceToDevice, m->stream));
    return ORBFE_OK;
}

// Group g grown to `cap` elements: new buffers, the default fill, the live prefix of the columns
// that keep their contents, one synchronise.
int store_grow(orbfe_map* m, int g, int cap) {
    ColumnGroup& G = m->group[g];
    if (cap <= G.alloc) return ORBFE_OK;
    DevBuf nb[kMapCols];
    int st;
    for (int c = 0; c < kMapCols; ++c) {
        const MapColumn& C = kMapColumns[c];
        if (C.group != g) continue;
        if ((st = store_regrow(m, m->col[c], nb[c], (size_t)C.per, C.keep ? G.covered : 0, cap, C.fill)))
            return st;
    }
    ORBFE_HIP(hipStreamSynchronize(m->stream));
    for (int c = 0; c < kMapCols; ++c)
        if (kMapColumns[c].group == g) m->col[c] = std::move(nb[c]);
    G.alloc = cap;
    return ORBFE_OK;
}

// Group g covers n elements, the new ones at their defaults: the capacity doubles from `start`.
int store_cover(orbfe_map* m, int g, int n, int start) {
    int st;
    if ((st = store_grow(m, g, m->group[g].capacity_for(n, start)))) return st;
    m->group[g].cover(n);
    return ORBFE_OK;
}

// A pool regrown to n elements, the first `keep` kept; synchronous.
int store_grow_pool(orbfe_map* m, MapPool& p, size_t per, long long keep, long long n, MapFill f) {
    if (n <= p.alloc) return ORBFE_OK;
    DevBuf nb;
    int st;
    if ((st = store_regrow(m, p.buf, nb, per, keep, n, f))) return st;
    ORBFE_HIP(hipStreamSynchronize(m->stream));
    p.buf = std::move(nb);
    p.alloc = n;
    return ORBFE_OK;
}

// The keypoint pools hold what kf_mp's pool holds; what nobody set reads its default.
int store_side_pools(orbfe_map* m) {
    int st;
    const SidePoolPlan f = side_pool_plan(m->kf_mp, m->feat_pool.alloc);
    if ((st = store_grow_pool(m, m->feat_pool, 1, f.keep, f.alloc, kFillFeat))) return st;
    const SidePoolPlan d = side_pool_plan(m->kf_mp, m->depth_pool.alloc);
    return store_grow_pool(m, m->depth_pool, sizeof(float), d.keep, d.alloc, kFillDepth);
}

// Everything back at its default for an empty map; the buffers stay.  Enqueued only.
int store_reset(orbfe_map* m) {
    int st;
    for (int c = 0; c < kMapCols; ++c) {
        const MapColumn& C = kMapColumns[c];
        if (C.keep && (st = store_fill(m, m->col[c].p, (size_t)C.per, m->group[C.group].covered, C.fill)))
            return st;
    }
    for (ColumnGroup& G : m->group) G.covered = 0;
    if ((st = store_fill(m, m->feat_pool.buf.p, 1, side_pool_plan(m->kf_mp, m->feat_pool.alloc).keep, kFillFeat)))
        return st;
    if ((st = store_fill(m, m->depth_pool.buf.p, sizeof(float),
                         side_pool_plan(m->kf_mp, m->depth_pool.alloc).keep, kFillDepth)))
        return st;
    if ((st = store_fill(m, m->kdesc_pool.buf.p, kMapDescBytes, side_pool_plan(m->kf_mp, m->kdesc_pool.alloc).keep,
                         kFillZero)))
        return st;
    m->kf_mp.reset();
    m->kf_ch.reset();
    m->mp_obs.reset();
    m->cov.reset();
    return ORBFE_OK;
}

// A staging buffer of at least n elements, borrowed until the next borrow of the same role.
template <class T>
int store_borrow(orbfe_map* m, int role, size_t n, T*& p) {
    const int st = m->stage[role].ensure(sizeof(T) * std::max<size_t>(n, 1));
    p = m->stage[role].as<T>();
    return st;
}

// The pinned block's tail holds n ints.  Reallocated between calls only: no kernel that writes
// the block is in flight when an entry point gets here, and the launches come after.
int store_pin_reserve(orbfe_map* m, size_t n) {
    if (m->pin && n <= m->pin_tail) return ORBFE_OK;
    if (m->pin) hipHostFree(m->pin);
    m->pin = m->pin_dev = nullptr;
    m->pin_tail = 0;
    size_t a = 1024;
    while (a < n) a *= 2;
    void* p = nullptr;
    void* dp = nullptr;
    if (hipHostMalloc(&p, sizeof(int) * (kResTail + a), hipHostMallocDefault) != hipSuccess) return ORBFE_ERR_NOMEM;
    if (hipHostGetDevicePointer(&dp, p, 0) != hipSuccess) {
        hipHostFree(p);
        return ORBFE_ERR_NOMEM;
    }
    m->pin = static_cast<int*>(p);
    m->pin_dev = static_cast<int*>(dp);
    m->pin_tail = a;
    return ORBFE_OK;
}

// The row writes `w` into table `r` (and its side pool, if `side`): regions, the pools' growth,
// one upload, one scatter launch, one synchronise.
int store_put_rows(orbfe_map* m, RowTable& r, MapPool& pool, int off_col, int len_col,
                   const std::vector<MapRowWrite>& w, MapPool* side = nullptr) {
    if (w.empty()) return ORBFE_OK;
    std::vector<RowNeed> need(w.size());
    size_t total = 0;
    for (size_t i = 0; i < w.size(); ++i) {
        need[i] = {w[i].row, 0, w[i].new_len};
        total += (size_t)w[i].n;
    }
    const RowPlan plan = r.plan(need);
    std::vector<MapRowItem> items(w.size());
    std::vector<int> data((side ? 2 : 1) * total);
    size_t at = 0;
    for (size_t i = 0; i < w.size(); ++i) {
        const MapRowWrite& x = w[i];
        items[i] = {r.off[x.row] + x.first, r.off[x.row], (int)at, x.n, x.row, r.len[x.row]};
        if (x.n) std::memcpy(data.data() + at, x.data, sizeof(int) * (size_t)x.n);
        if (side && x.n) std::memcpy(data.data() + total + at, x.data2, sizeof(int) * (size_t)x.n);
        at += (size_t)x.n;
    }
    int st;
    // whole-row writes only: of a row that moves nothing survives, so the used prefix is enough
    if ((st = store_grow_pool(m, pool, sizeof(int), r.used, plan.alloc, kFillZero))) return st;
    if (side && (st = store_grow_pool(m, *side, sizeof(int), r.used, plan.alloc, kFillZero))) return st;
    r.commit(plan);
    int* d_data;
    MapRowItem* d_items;
    if ((st = store_borrow(m, kStageVals, data.size(), d_data))) return st;
    if ((st = store_borrow(m, kStageItems, items.size(), d_items))) return st;
    if (!data.empty())
        ORBFE_HIP(hipMemcpyAsync(d_data, data.data(), sizeof(int) * data.size(), hipMemcpyHostToDevice, m->stream));
    ORBFE_HIP(hipMemcpyAsync(d_items, items.data(), sizeof(MapRowItem) * items.size(), hipMemcpyHostToDevice,
                             m->stream));
    const int n_items = (int)items.size();
    hipLaunchKernelGGL(map_rows_kernel, dim3((n_items + 3) / 4), dim3(256), 0, m->stream, n_items, d_items,
                       d_data, pool.buf.as<int>(), d_data + total, side ? side->buf.as<int>() : nullptr,
                       m->at<long long>(off_col), m->at<int>(len_col));
    ORBFE_HIP(hipGetLastError());
    ORBFE_HIP(hipStreamSynchronize(m->stream));  // the staging vectors are this call's
    return ORBFE_OK;
}

int map_put_kf_mp(orbfe_map* m, const std::vector<MapRowWrite>& w) {
    return store_put_rows(m, m->kf_mp, m->kf_mp_pool, kColKfMpOff, kColKfMpLen, w);
}
int map_put_kf_ch(orbfe_map* m, const std::vector<MapRowWrite>& w) {
    return store_put_rows(m, m->kf_ch, m->kf_ch_pool, kColKfChOff, kColKfChLen, w);
}
int map_put_mp_obs(orbfe_map* m, const std::vector<MapRowWrite>& w) {
    return store_put_rows(m, m->mp_obs, m->mp_obs_pool, kColMpObsOff, kColMpObsLen, w, &m->mp_idx_pool);
}

// The n slots staged for one launch; all in range (checked by the caller).
int store_stage_slots(orbfe_map* m, int n, const int32_t* slots, int*& d_slots) {
    int st;
    if ((st = store_borrow(m, kStageSlots, (size_t)n, d_slots))) return st;
    ORBFE_HIP(hipMemcpyAsync(d_slots, slots, sizeof(int) * (size_t)n, hipMemcpyHostToDevice, m->stream));
    return ORBFE_OK;
}

// dst[slots[i]] = vals[i] (or `value`) for n slots; one launch, one synchronise.
template <class T>
int store_set(orbfe_map* m, T* dst, int n, const int32_t* slots, const T* vals, T value = T()) {
    if (!n) return ORBFE_OK;
    int st;
    int* d_slots;
    T* d_vals = nullptr;
    if ((st = store_stage_slots(m, n, slots, d_slots))) return st;
    if (vals) {
        if ((st = store_borrow(m, kStageVals, (size_t)n, d_vals))) return st;
        ORBFE_HIP(hipMemcpyAsync(d_vals, vals, sizeof(T) * (size_t)n, hipMemcpyHostToDevice, m->stream));
    }
    hipLaunchKernelGGL(store_set_kernel<T>, dim3((n + 255) / 256), dim3(256), 0, m->stream, n, d_slots,
                       static_cast<const T*>(d_vals), value, dst);
    ORBFE_HIP(hipGetLastError());
    ORBFE_HIP(hipStreamSynchronize(m->stream));
    return ORBFE_OK;
}

// out[i] = src[slots[i]] for n slots; one launch, one copy back, one synchronise.
template <class T>
int store_get(orbfe_map* m, const T* src, int n, const int32_t* slots, T* out) {
    if (!n) return ORBFE_OK;
    int st;
    int* d_slots;
    T* d_out;
    if ((st = store_stage_slots(m, n, slots, d_slots))) return st;
    if ((st = store_borrow(m, kStageOut, (size_t)n, d_out))) return st;
    hipLaunchKernelGGL(store_get_kernel<T>, dim3((n + 255) / 256), dim3(256), 0, m->stream, n, d_slots, src,
                       d_out);
    ORBFE_HIP(hipGetLastError());
    ORBFE_HIP(hipMemcpyAsync(out, d_out, sizeof(T) * (size_t)n, hipMemcpyDeviceToHost, m->stream));
    ORBFE_HIP(hipStreamSynchronize(m->stream));
    return ORBFE_OK;
}

// dst[slots[i]] += amounts[i] (or `amount`) for n slots; one launch, one synchronise.
int store_add(orbfe_map* m, int* dst, int n, const int32_t* slots, const int* amounts, int amount = 0) {
    if (!n) return ORBFE_OK;
    int st;
    int* d_slots;
    int* d_amounts = nullptr;
    if ((st = store_stage_slots(m, n, slots, d_slots))) return st;
    if (amounts) {
        if ((st = store_borrow(m, kStageVals, (size_t)n, d_amounts))) return st;
        ORBFE_HIP(hipMemcpyAsync(d_amounts, amounts, sizeof(int) * (size_t)n, hipMemcpyHostToDevice, m->stream));
    }
    hipLaunchKernelGGL(store_add_kernel, dim3((n + 255) / 256), dim3(256), 0, m->stream, n, d_slots,
                       static_cast<const int*>(d_amounts), amount, dst);
    ORBFE_HIP(hipGetLastError());
    ORBFE_HIP(hipStreamSynchronize(m->stream));
    return ORBFE_OK;
}

// The call error word cleared ahead of a call's launches / read back after them (synchronises).
int store_clear_err(orbfe_map* m) {
    ORBFE_HIP(hipMemsetAsync(m->call_err(), 0, sizeof(int), m->stream));
    return ORBFE_OK;
}
int store_read_err(orbfe_map* m, int& err) {
    ORBFE_HIP(hipMemcpyAsync(&err, m->call_err(), sizeof(int), hipMemcpyDeviceToHost, m->stream));
    ORBFE_HIP(hipStreamSynchronize(m->stream));
    return ORBFE_OK;
}

// The covisibility group covers every keyframe of the map; made by the first call that gets here.
int cov_ready(orbfe_map* m) {
    int st;
    if ((st = store_cover(m, kGroupCovis, m->n_kf, 16))) return st;
    m->cov.cover((size_t)m->n_kf);
    m->h_nw.resize((size_t)m->n_kf, 0);
    m->h_no.resize((size_t)m->n_kf, 0);
    return ORBFE_OK;
}

// The culling groups cover every point and keyframe of the map, at the core groups' capacities.
int cull_ready(orbfe_map* m) {
    int st;
    if (m->n_mp > m->group[kGroupCullMp].alloc && (st = store_grow(m, kGroupCullMp, m->group[kGroupCoreMp].alloc)))
        return st;
    m->group[kGroupCullMp].cover(m->n_mp);
    if (m->n_kf > m->group[kGroupCullKf].alloc && (st = store_grow(m, kGroupCullKf, m->group[kGroupCoreKf].alloc)))
        return st;
    m->group[kGroupCullKf].cover(m->n_kf);
    m->h_feat.resize((size_t)m->n_kf);
    m->h_th_depth.resize((size_t)m->n_kf, 0.f);
    m->h_not_erase.resize((size_t)m->n_kf, 0);
    m->h_to_erase.resize((size_t)m->n_kf, 0);
    return ORBFE_OK;
}

// The refresh groups (mpRefKF; camera centres and descriptor flags) cover every point and keyframe
// of the map, at the core groups' capacities.  ref_made(): whether any call has made mpRefKF.
bool ref_made(const orbfe_map* m) { return m->group[kGroupRefMp].alloc > 0; }
int ref_ready_mp(orbfe_map* m) {
    int st;
    if (m->n_mp > m->group[kGroupRefMp].alloc && (st = store_grow(m, kGroupRefMp, m->group[kGroupCoreMp].alloc)))
        return st;
    m->group[kGroupRefMp].cover(m->n_mp);
    return ORBFE_OK;
}
int ref_ready_kf(orbfe_map* m) {
    int st;
    if (m->n_kf > m->group[kGroupRefKf].alloc && (st = store_grow(m, kGroupRefKf, m->group[kGroupCoreKf].alloc)))
        return st;
    m->group[kGroupRefKf].cover(m->n_kf);
    m->h_desc_set.resize((size_t)m->n_kf, 0);
    return ORBFE_OK;
}

// The descriptor pool holds what kf_mp's pool holds; rows nobody set read zero.
int store_desc_pool(orbfe_map* m) {
    const SidePoolPlan p = side_pool_plan(m->kf_mp, m->kdesc_pool.alloc);
    return store_grow_pool(m, m->kdesc_pool, kMapDescBytes, p.keep, p.alloc, kFillZero);
}

int map_reset_ctl(orbfe_map* m) {
    int h[kCtlWords] = {0};
    h[kCtlRef] = -1;
    ORBFE_HIP(hipMemcpyAsync(m->ctl.p, h, sizeof h, hipMemcpyHostToDevice, m->stream));
    ORBFE_HIP(hipStreamSynchronize(m->stream));
    return ORBFE_OK;
}

}  // namespace

extern "C" {

orbfe_map* orbfe_map_create(int device, int kf_hint, int mp_hint, int* status) {
    int st = kf_hint < 0 || mp_hint < 0 ? ORBFE_ERR_ARG : check_device(device);
    orbfe_map* m = nullptr;
    if (st == ORBFE_OK) {
        try {
            DeviceGuard dg(device);
            m = new orbfe_map();
            m->device = device;
            if (hipStreamCreateWithFlags(&m->own, hipStreamNonBlocking) != hipSuccess) st = ORBFE_ERR_HIP;
            m->stream = m->own;
            if (st == ORBFE_OK) st = store_pin_reserve(m, kMapListCap);
            if (st == ORBFE_OK) st = m->ctl.ensure(sizeof(int) * kCtlWords);
            if (st == ORBFE_OK) st = m->touched.ensure(sizeof(int) * kMapMaxVoted);
            if (st == ORBFE_OK) st = m->local_kf.ensure(sizeof(int) * kMapListCap);
            if (st == ORBFE_OK) st = m->blk.ensure(sizeof(int) * (size_t)kMapListCap * kMapChunks);
            if (st == ORBFE_OK) st = map_reset_ctl(m);
            if (st == ORBFE_OK) st = store_grow(m, kGroupCoreKf, std::max(kf_hint, 16));
            if (st == ORBFE_OK) st = store_grow(m, kGroupCoreMp, std::max(mp_hint, 1024));
        } catch (const std::bad_alloc&) {
            st = ORBFE_ERR_NOMEM;
        } catch (...) {
            st = ORBFE_ERR_HIP;
        }
    }
    if (st != ORBFE_OK && m) {
        delete m;
        m = nullptr;
    }
    if (status) *status = st;
    return m;
}

void orbfe_map_destroy(orbfe_map* m) {
    if (!m) return;
    DeviceGuard dg(m->device);
    if (m->stream) hipStreamSynchronize(m->stream);
    delete m;
}

int orbfe_map_set_stream(orbfe_map* m, void* hip_stream) {
    if (!m) return ORBFE_ERR_ARG;
    DeviceGuard dg(m->device);
    hipStreamSynchronize(m->stream);
    m->stream = hip_stream ? static_cast<hipStream_t>(hip_stream) : m->own;
    return ORBFE_OK;
}

int orbfe_map_clear(orbfe_map* m) {
    if (!m) return ORBFE_ERR_ARG;
    return map_guarded(m, [&]() {
        int st;
        if ((st = store_reset(m))) return st;
        m->n_kf = m->n_mp = m->max_slots = 0;
        m->by_key.clear();
        m->h_key.clear();
        m->h_obs.clear();
        m->h_idx.clear();
        m->n_unknown = 0;
        m->h_local.clear();
        m->h_ref = -1;
        m->h_n_local_mp = 0;
        m->h_nw.clear();
        m->h_no.clear();
        m->h_feat.clear();
        m->h_th_depth.clear();
        m->h_not_erase.clear();
        m->h_to_erase.clear();
        m->h_scale.clear();
        m->h_desc_set.clear();
        return map_reset_ctl(m);
    });
}

int orbfe_map_size(const orbfe_map* m, int32_t* n_keyframes, int32_t* n_points) {
    if (!m) return ORBFE_ERR_ARG;
    if (n_keyframes) *n_keyframes = m->n_kf;
    if (n_points) *n_points = m->n_mp;
    return ORBFE_OK;
}

}  // extern "C"
