// orbfe_grid.hip — the Frame grid (skaegy/ORBSLAM_MapSave src/Frame.cc) every projection matcher
// queries: the 64 x 48 cell table of Frame::AssignFeaturesToGrid as a CSR, and
// Frame::GetFeaturesInArea on it.  The matchers' first-wins ties depend on the exact item order,
// so every grid of the library -- the stand-alone builder's and the one sbp_local_fused_kernel
// (orbfe_greedy.hip) keeps in its own LDS -- is made of the pieces below.
//
//   grid_cell / grid_scan / grid_sort   PosInGrid, counts -> cursors, per-cell index order
//   grid_kernel           Frame::AssignFeaturesToGrid (Frame.cc:341-356) as a CSR, one
//                         workgroup per frame of a batch
//   cell_window           the clipped cell window of GetFeaturesInArea
//   features_in_area(_wave)  Frame::GetFeaturesInArea (Frame.cc:445-498), a thread / a wave per
//                         query
//   fia_*_kernel          the same as a batch of queries (the grid's parity probe)
//
// and, at the end, the pieces the matcher kernels on top of it are made of, each written once:
//
//   CandArgs / CandSink   the candidate-list shell of every *_cand_kernel
//   pose_apply            the 3 x 4 pose product
//   kMin/kMaxDistInvariance / predict_level / level_in_pyramid
//                         MapPoint's distance invariance and PredictScale
//   wave_first_min        first-wins (distance, rank) minimum over a wave
//   readlane_desc         a descriptor pair broadcast from one lane
//   last_workgroup        "the last workgroup to finish runs the tail"
#include <hip/hip_runtime.h>

#include "../../include/orbfe.h"
#include "orbfe_device.hpp"

namespace orbfe {

constexpr int kGridCols = 64, kGridRows = 48;  // FRAME_GRID_COLS/ROWS (Frame.h:37-38)
constexpr int kGridCells = kGridCols * kGridRows;

struct DevFrame {
    const orbfe_keypoint* k;
    const uint4* desc;  // 2 x uint4 per keypoint
    const float* ur;    // NULL: monocular
    int n;
    float minx, maxx, miny, maxy, gwi, ghi;
    const int* cstart;  // kGridCells + 1
    const int* citems;
};

// A frame view over device arrays.
inline DevFrame dev_frame(const orbfe_frame_view* v, const orbfe_keypoint* k, const uint4* desc,
                          const float* ur, const int* cstart, const int* citems) {
    return DevFrame{k, desc, ur, v->n,
                    v->min_x, v->max_x, v->min_y, v->max_y, v->grid_w_inv, v->grid_h_inv,
                    cstart, citems};
}

// Frame::PosInGrid (Frame.cc:500-510): the cell mGrid[ix][iy] of a keypoint as ix * kGridRows + iy,
// -1 outside the grid.
__device__ __forceinline__ int grid_cell(float x, float y, float minx, float miny, float gwi,
                                         float ghi) {
    const int gx = (int)roundf((x - minx) * gwi);
    const int gy = (int)roundf((y - miny) * ghi);
    if (gx < 0 || gx >= kGridCols || gy < 0 || gy >= kGridRows) return -1;
    return gx * kGridRows + gy;
}

// The grid's LDS table is cs[kGridCells + 1] with cs[0] = 0 and the cell counters at cur = cs + 1.
// grid_scan turns the counts cur[c] into the cells' starts, which the fill then uses as cursors
// (slot = atomicAdd(&cur[c], 1)); after the fill cur[c] is the end of cell c, that is the start
// of cell c + 1, so cs[0 .. kGridCells] is the finished CSR row table with no further pass.
// Every thread of the block calls it, after a barrier behind the counting; it ends with a
// barrier.  Returns the item total.
template <int BLOCK>
__device__ __forceinline__ int grid_scan(int* cur, int* tmp) {
    constexpr int PER = (kGridCells + BLOCK - 1) / BLOCK;
    int local[PER], sum = 0;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        const int c = threadIdx.x * PER + j;
        local[j] = c < kGridCells ? cur[c] : 0;
        sum += local[j];
    }
    int total;
    int off = block_exclusive_scan<BLOCK>(sum, tmp, total);
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        const int c = threadIdx.x * PER + j;
        if (c < kGridCells) cur[c] = off;
        off += local[j];
    }
    __syncthreads();
    return total;
}

// AssignFeaturesToGrid pushes keypoints in index order (Frame.cc:341-356); the fill's atomics
// do not, so every cell [cs[c], cs[c + 1]) of items (LDS or global) is sorted by index.  Cells
// hold a few items: an insertion sort per cell, cells dealt over the block's threads.
template <int BLOCK>
__device__ __forceinline__ void grid_sort(const int* cs, int* items) {
    for (int c = threadIdx.x; c < kGridCells; c += BLOCK) {
        const int s = cs[c], e = cs[c + 1];
        for (int q = s + 1; q < e; ++q) {
            const int v = items[q];
            int b = q - 1;
            while (b >= s && items[b] > v) {
                items[b + 1] = items[b];
                --b;
            }
            items[b + 1] = v;
        }
    }
}

constexpr int kGridBlock = 1024;
constexpr int kGridPer = 8;                         // keypoints per thread held in registers
constexpr int kGridLdsMax = kGridBlock * kGridPer;  // 8192: the items list fits LDS (32 KB)
// Frame::AssignFeaturesToGrid (Frame.cc:341-356) of frame f = blockIdx.x as a CSR at
// cstart + f * (kGridCells + 1) / citems + f * cap, over the keypoints at keys + f * keys_pitch.
// The frame holds min(n_kp[f], kp_max) keypoints, or kp_max with n_kp NULL.
// Up to kGridLdsMax keypoints the cell of every keypoint stays in registers and the items list
// is filled, ordered and only then copied out of LDS, so no step waits on a chain of dependent
// global loads; above, the cells are recomputed for the fill and the list is filled and ordered
// in place in citems.
__global__ __launch_bounds__(kGridBlock) void grid_kernel(const orbfe_keypoint* keys,
                                                          long long keys_pitch, const int* n_kp,
                                                          int kp_max, float minx, float miny,
                                                          float gwi, float ghi, int* cstart,
                                                          int* citems, int cap) {
    __shared__ int cs[kGridCells + 1];
    __shared__ int items[kGridLdsMax];
    __shared__ int tmp[kGridBlock / 64 + 1];
    const int f = blockIdx.x, tid = threadIdx.x;
    const orbfe_keypoint* k = keys + f * keys_pitch;
    const int n = n_kp ? min(max(n_kp[f], 0), kp_max) : kp_max;
    cstart += (size_t)f * (kGridCells + 1);
    citems += (size_t)f * cap;
    int* cur = cs + 1;
    for (int c = tid; c <= kGridCells; c += kGridBlock) cs[c] = 0;
    __syncthreads();
    const bool lds = n <= kGridLdsMax;
    // lds: cells of keypoints tid + j * kGridBlock, slots j < nslot in use (a small frame leaves
    // the unrolled slots by one branch)
    int mine[kGridPer];
    const int nslot = (n + kGridBlock - 1) / kGridBlock;
    if (lds) {
#pragma unroll
        for (int j = 0; j < kGridPer; ++j) {
            if (j >= nslot) break;
            const int i = tid + j * kGridBlock;
            mine[j] = i < n ? grid_cell(k[i].x, k[i].y, minx, miny, gwi, ghi) : -1;
            if (mine[j] >= 0) atomicAdd(&cur[mine[j]], 1);
        }
    } else {
        for (int i = tid; i < n; i += kGridBlock) {
            const int c = grid_cell(k[i].x, k[i].y, minx, miny, gwi, ghi);
            if (c >= 0) atomicAdd(&cur[c], 1);
        }
    }
    __syncthreads();
    const int total = grid_scan<kGridBlock>(cur, tmp);
    // the row table goes out now, under the fill and the sort, not behind them
    for (int c = tid; c < kGridCells; c += kGridBlock) cstart[c] = cur[c];
    if (tid == 0) cstart[kGridCells] = total;
    __syncthreads();  // the fill moves the cursors
    if (lds) {
#pragma unroll
        for (int j = 0; j < kGridPer; ++j) {
            if (j >= nslot) break;
            if (mine[j] >= 0) items[atomicAdd(&cur[mine[j]], 1)] = tid + j * kGridBlock;
        }
        __syncthreads();
        grid_sort<kGridBlock>(cs, items);
        __syncthreads();
        for (int i = tid; i < total; i += kGridBlock) citems[i] = items[i];
    } else {
        for (int i = tid; i < n; i += kGridBlock) {
            const int c = grid_cell(k[i].x, k[i].y, minx, miny, gwi, ghi);
            if (c >= 0) citems[atomicAdd(&cur[c], 1)] = i;
        }
        __syncthreads();
        grid_sort<kGridBlock>(cs, citems);
    }
}

// The cells Frame::GetFeaturesInArea (Frame.cc:445-498) visits for (x, y, r): columns cx0 ..,
// rows cy0 .. cy0 + ny - 1, ncell cells in ix-major, iy order; empty when the window lies
// outside the grid (the reference's four early returns).
struct CellWindow {
    int cx0, cy0, ny, ncell;
    bool empty;
    __device__ __forceinline__ int cell(int t) const {  // t-th cell of the window
        return (cx0 + t / ny) * kGridRows + cy0 + t % ny;
    }
};
__device__ __forceinline__ CellWindow cell_window(const DevFrame& F, float x, float y, float r) {
    const int cx0 = max(0, (int)floorf((x - F.minx - r) * F.gwi));
    const int cx1 = min(kGridCols - 1, (int)ceilf((x - F.minx + r) * F.gwi));
    const int cy0 = max(0, (int)floorf((y - F.miny - r) * F.ghi));
    const int cy1 = min(kGridRows - 1, (int)ceilf((y - F.miny + r) * F.ghi));
    CellWindow w;
    w.cx0 = cx0;
    w.cy0 = cy0;
    w.ny = cy1 - cy0 + 1;
    w.ncell = (cx1 - cx0 + 1) * w.ny;
    w.empty = cx0 >= kGridCols || cx1 < 0 || cy0 >= kGridRows || cy1 < 0;
    return w;
}

// Frame::GetFeaturesInArea (Frame.cc:445-498): visits candidates in ix-major, iy, insertion
// order and calls fn(idx) for each.
template <class Fn>
__device__ __forceinline__ void features_in_area(const DevFrame& F, float x, float y, float r,
                                                 int min_level, int max_level, Fn fn) {
    const CellWindow w = cell_window(F, x, y, r);
    if (w.empty) return;
    const bool check = min_level > 0 || max_level >= 0;
    for (int ix = w.cx0, xe = w.cx0 + w.ncell / w.ny; ix < xe; ++ix)
        for (int iy = w.cy0; iy < w.cy0 + w.ny; ++iy) {
            const int c = ix * kGridRows + iy;
            for (int e = F.cstart[c]; e < F.cstart[c + 1]; ++e) {
                const int idx = F.citems[e];
                const orbfe_keypoint kp = F.k[idx];
                if (check) {
                    if (kp.octave < min_level) continue;
                    if (max_level >= 0 && kp.octave > max_level) continue;
                }
                if (fabsf(kp.x - x) < r && fabsf(kp.y - y) < r) fn(idx);
            }
        }
}

// Wave-cooperative GetFeaturesInArea for one query per wave (every lane passes the same query):
// lane t takes cell t of the window in the reference's ix-major, iy order (64 cells per
// step), counts its passing items, and an exclusive wave scan of the counts places every
// candidate at its reference rank; emit(idx, rank) runs on the lane owning the candidate.
// Returns the candidate count (wave-uniform).  keep(idx) is an extra per-candidate filter.
template <class Keep, class Emit>
__device__ __forceinline__ int features_in_area_wave(const DevFrame& F, float x, float y, float r,
                                                     int min_level, int max_level, Keep keep,
                                                     Emit emit) {
    const int lane = threadIdx.x & 63;
    const CellWindow w = cell_window(F, x, y, r);
    if (w.empty) return 0;
    const bool check = min_level > 0 || max_level >= 0;
    auto pass = [&](int idx) {
        const orbfe_keypoint kp = F.k[idx];
        if (check) {
            if (kp.octave < min_level) return false;
            if (max_level >= 0 && kp.octave > max_level) return false;
        }
        return fabsf(kp.x - x) < r && fabsf(kp.y - y) < r && keep(idx);
    };
    int total = 0;
    for (int c0 = 0; c0 < w.ncell; c0 += 64) {
        const int t = c0 + lane;
        int e0 = 0, e1 = 0, n = 0;
        if (t < w.ncell) {
            const int c = w.cell(t);
            e0 = F.cstart[c];
            e1 = F.cstart[c + 1];
            for (int e = e0; e < e1; ++e) n += pass(F.citems[e]);
        }
        const int inc = wave_inclusive_sum(n);
        int rank = total + inc - n;
        if (n)
            for (int e = e0; e < e1; ++e) {
                const int idx = F.citems[e];
                if (pass(idx)) emit(idx, rank++);
            }
        total += __shfl(inc, 63, 64);
    }
    return total;
}

// Exclusive scan of counts[0..n) into off[0..n], single workgroup.
__global__ __launch_bounds__(1024) void scan_kernel(const int* counts, int n, int* off) {
    __shared__ int tmp[1024 / 64 + 1];
    int run = 0;
    for (int base = 0; base < n; base += 1024) {
        const int i = base + threadIdx.x;
        const int v = i < n ? counts[i] : 0;
        int t;
        const int ex = block_exclusive_scan<1024>(v, tmp, t);
        if (i < n) off[i] = run + ex;
        run += t;
    }
    if (threadIdx.x == 0) off[n] = run;
}

// ---------------------------------------------------------------------------------------------
// Frame::GetFeaturesInArea (Frame.cc:445-498) as a batch of queries — the parity probe of the
// grid (orbfe_features_in_area): thread-per-query (features_in_area) and wave-per-query
// (features_in_area_wave, which the matchers use: SearchForInitialization, SearchByProjection's
// local-map / last-frame / keyframe forms) write each query's candidates in the reference's
// order to items[off[q] ..).
struct FiaArgs {
    DevFrame f;
    int nq;
    const float* x;
    const float* y;
    const float* r;
    const int* lo;
    const int* hi;
    int* cnt;
    const int* off;
    int* items;
};
template <bool FILL>
__global__ __launch_bounds__(256) void fia_thread_kernel(FiaArgs a) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= a.nq) return;
    const int o = FILL ? a.off[q] : 0;
    int n = 0;
    features_in_area(a.f, a.x[q], a.y[q], a.r[q], a.lo[q], a.hi[q], [&](int idx) {
        if (FILL) a.items[o + n] = idx;
        ++n;
    });
    if (!FILL) a.cnt[q] = n;
}
template <bool FILL>
__global__ __launch_bounds__(256) void fia_wave_kernel(FiaArgs a) {
    const int q = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= a.nq) return;
    const int o = FILL ? a.off[q] : 0;
    const int n = features_in_area_wave(
        a.f, a.x[q], a.y[q], a.r[q], a.lo[q], a.hi[q], [](int) { return true; },
        [&](int idx, int rank) {
            if (FILL) a.items[o + rank] = idx;
        });
    if (!FILL && (threadIdx.x & 63) == 0) a.cnt[q] = n;
}

// ---------------------------------------------------------------------------------------------
// The pieces the matcher kernels share (orbfe_match / _fuse / _bow / _loop / _triangulate /
// _greedy.hip).  The build keeps -ffp-contract=off and every float expression below is
// parenthesised as the reference evaluates it: a rounding detail or a bound is fixed here, once.
// What differs between the searches by the reference's own choice -- how 1/z is formed, the
// in-image and viewing tests, the level windows, the acceptance thresholds -- stays at the call
// sites ("One shell for the candidate kernels").

// The candidate lists a *_cand_kernel writes, filled in by the host's candidate builder
// (orbfe_match_api.hip): CSR lists (count -> scan -> fill) or kfix fixed slots per query.
struct CandArgs {
    long long cand_cap;  // fill writes only lists that end within the capacity
    int* cnt;            // per query
    const int* off;      // queries + 1
    int2* cand;          // (index, payload): the distance, or dist | octave << 16 (local map)
    int kfix;            // fixed-slot form: candidate slots per query
    int* ovf;            // fixed-slot form: queries with more candidates than kfix
};

// The shell of a candidate kernel, one wave per query q.  kMode 0: count the candidates,
// 1: fill the CSR lists (after the scan), 2: the fixed-slot form in one pass -- the first kfix
// candidates of query q at q * kfix, min(n, kfix) in cnt[q], and a query with more raises *ovf
// (the host then reruns the call on the CSR path).
template <int kMode>
struct CandSink {
    const CandArgs& c;
    const int q;
    // fill: the query's list ends within the capacity (else the host reruns with more)
    __device__ __forceinline__ bool room() const { return kMode != 1 || c.off[q + 1] <= c.cand_cap; }
    __device__ __forceinline__ int2* out() const {
        return kMode == 1 ? c.cand + c.off[q] : kMode == 2 ? c.cand + (size_t)q * c.kfix : nullptr;
    }
    // the candidate of rank `rank` (features_in_area_wave's emit), on the lane that owns it;
    // payload() -- the descriptor loads and the distance -- runs only for a candidate that is
    // stored, so the count mode's walk stays free of them
    template <class Payload>
    __device__ __forceinline__ void put(int2* out, int rank, int idx, Payload payload) const {
        if (kMode == 1 || (kMode == 2 && rank < c.kfix)) out[rank] = make_int2(idx, payload());
    }
    // the query's n candidates are through (n = 0: a query that is not searched)
    __device__ __forceinline__ void finish(int n) const {
        const bool lead = (threadIdx.x & 63) == 0;  // the lane that writes the query's words
        if (kMode == 0 && lead) c.cnt[q] = n;
        if (kMode == 2 && lead) {
            c.cnt[q] = min(n, c.kfix);
            if (n > c.kfix) atomicAdd(c.ovf, 1);
        }
    }
};

// pc = [R|t] P for a row-major 3 x 4 pose T, each row summed left to right as cv::Mat's float
// product followed by + t does.
__device__ __forceinline__ void pose_apply(const float* T, const float* P, float* pc) {
#pragma unroll
    for (int r = 0; r < 3; ++r)
        pc[r] = ((T[4 * r] * P[0] + T[4 * r + 1] * P[1]) + T[4 * r + 2] * P[2]) + T[4 * r + 3];
}

// MapPoint::GetMinDistanceInvariance / GetMaxDistanceInvariance (MapPoint.cc:621-631): the
// factors on mfMinDistance / mfMaxDistance.  The bounds and the test on them,
// !(dist < dmin || dist > dmax), are written out in each search's chain of tests: as constants
// they leave every kernel's code as it was (a helper returning the bool made frustum_kernel
// branch, and even one returning a bound moved its registers).
constexpr float kMinDistInvariance = 0.8f, kMaxDistInvariance = 1.2f;

// MapPoint::PredictScale (MapPoint.cc:633-642) before its clamp, which none of the callers has:
// the log in double, the quotient in float.
__device__ __forceinline__ int predict_level(float maxd, float dist, float log_scale) {
    const float ratio = maxd / dist;
    return (int)ceilf((float)log((double)ratio) / log_scale);
}

// mvScaleFactors[lvl] is in range; otherwise the reference reads past the vector and the wave
// raises ORBFE_ERR_UNSUPPORTED in *status.
__device__ __forceinline__ bool level_in_pyramid(int lvl, int nlevels, int* status) {
    if (lvl < 0 || lvl >= nlevels) {
        if ((threadIdx.x & 63) == 0) atomicExch(status, ORBFE_ERR_UNSUPPORTED);
        return false;
    }
    return true;
}

// The wave's smallest key = distance << 32 | rank and the idx that came with it, into every
// lane: the first candidate in rank order among equal distances, as a strict-< loop picks.
// (The reduction runs on copies: on the references themselves fuse_search_kernel grew by 23
// instructions and its batch row by 0.8 %.)
__device__ __forceinline__ void wave_first_min(unsigned long long& key_io, int& idx_io) {
    unsigned long long key = key_io;
    int idx = idx_io;
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
        const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)key, s, 64);
        const unsigned hi = (unsigned)__shfl_xor((int)(unsigned)(key >> 32), s, 64);
        const int oi = __shfl_xor(idx, s, 64);
        const unsigned long long c = ((unsigned long long)hi << 32) | lo;
        if (c < key) {
            key = c;
            idx = oi;
        }
    }
    key_io = key;
    idx_io = idx;
}

// The descriptor (my0, my1) of lane t into scalar registers (t is wave-uniform: v_readlane, no
// LDS round trip).
__device__ __forceinline__ void readlane_desc(const uint4& my0, const uint4& my1, int t, uint4& q0,
                                              uint4& q1) {
    q0 = make_uint4(__builtin_amdgcn_readlane(my0.x, t), __builtin_amdgcn_readlane(my0.y, t),
                    __builtin_amdgcn_readlane(my0.z, t), __builtin_amdgcn_readlane(my0.w, t));
    q1 = make_uint4(__builtin_amdgcn_readlane(my1.x, t), __builtin_amdgcn_readlane(my1.y, t),
                    __builtin_amdgcn_readlane(my1.z, t), __builtin_amdgcn_readlane(my1.w, t));
}

// True in every thread of the last of the grid's gridDim.x workgroups (of one blockIdx.y) to get
// here; *counter is 0 before the launch and counts them.  Every thread releases its own stores,
// the workgroup is counted behind a barrier, and the last one acquires everyone's: what the
// others wrote before their call is visible after it.  Every thread of the workgroup calls it,
// once per kernel.
__device__ __forceinline__ bool last_workgroup(int* counter) {
    __shared__ int last;
    __threadfence();
    __syncthreads();
    if (threadIdx.x == 0) last = atomicAdd(counter, 1) == (int)gridDim.x - 1;
    __syncthreads();
    if (!last) return false;
    __threadfence();
    return true;
}

}  // namespace orbfe
