// orbfe_internal.hpp — structs shared by the extractor kernels and their host orchestration.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <chrono>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/orbfe.h"

namespace orbfe {

constexpr int kMaxLevels = 16;

// FAST candidate / oct-tree key: x, y (12 bits each; level coords or coords relative to
// (16,16)) and the FAST score (8 bits).  Images are limited to 4096 x 4096.
__host__ __device__ __forceinline__ uint32_t pack_key(int x, int y, int s) {
    return ((uint32_t)y << 20) | ((uint32_t)x << 8) | (uint32_t)s;
}
__host__ __device__ __forceinline__ int key_x(uint32_t k) { return (int)((k >> 8) & 0xfff); }
__host__ __device__ __forceinline__ int key_y(uint32_t k) { return (int)(k >> 20); }
__host__ __device__ __forceinline__ int key_score(uint32_t k) { return (int)(k & 0xff); }

struct LevelGeo {
    int w, h, pitch;       // level size; row pitch inside the pyramid / blur slabs
    long long off;         // byte offset of the level inside a frame's slab
    int cell_begin, cell_end;
    int key_cap;           // sum of the level's cell capacities
    long long key_off;     // offset (keys) of the level inside a frame's key region
    int nfeat;             // mnFeaturesPerLevel[level]
    int nini;              // initial oct-tree nodes round(bw / bh) (542)
    float hx;              // (maxX - minX) / nIni (544)
    int bw, bh;            // maxBorderX - minBorderX, maxBorderY - minBorderY
    int ncap;              // oct-tree list capacity max(N + 4, 4 nIni + 4)
    int out_off;           // offset of the level inside a frame's oct-tree output
    float scale, size;     // mvScaleFactor[level], (int)(31 * scale)
};

struct Geo {
    int nlevels;
    long long key_total;   // keys per frame (all levels)
    int out_total;         // oct-tree output slots per frame (all levels)
    LevelGeo lv[kMaxLevels];
};

struct CellDesc {
    int level;
    int y0, y1, x0, x1;    // FAST ROI rows [y0,y1) cols [x0,x1) in level coords
    int cap;               // max keys the cell can emit
    long long slot;        // offset of the cell's keys inside a frame's cell-key region
};

struct LevelPtr {
    const uint8_t* base;   // frame 0, level origin
    long long fpitch;      // bytes between frames
    int pitch;             // bytes between rows
};

// The bounded wait on device-mapped pinned memory: until none of the n words at w (each written
// once, with release semantics at system scope, by a kernel on `stream`) holds `pending`.  Polls
// with acquire loads, so what the kernel wrote before a word is visible once the word is; past
// limit_us it synchronises the stream (which reports a failed kernel) and checks once more.
inline int wait_words(const int* w, int n, int pending, hipStream_t stream, int limit_us) {
    const auto t0 = std::chrono::steady_clock::now();
    for (int s = 0; s < n; ++s) {
        while (__atomic_load_n(w + s, __ATOMIC_ACQUIRE) == pending) {
            if (std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(limit_us)) {
                if (hipStreamSynchronize(stream) != hipSuccess) return ORBFE_ERR_HIP;
                for (; s < n; ++s)
                    if (__atomic_load_n(w + s, __ATOMIC_ACQUIRE) == pending) return ORBFE_ERR_HIP;
                return ORBFE_OK;
            }
            __builtin_ia32_pause();
        }
    }
    return ORBFE_OK;
}

// Pixels [0, n) of a w-pixel row that OpenCV 3.3's x86 SSE2 vertical kernels produce (the rest
// is the scalar tail): VResizeLinearVec_32s8u steps 16 while x <= w - 16, then 4 while
// x < w - 4; SymmColumnVec_32s8u steps 16 while i <= w - 16, then 4 while i <= w - 4.  Both
// are multiples of 4.
inline int sse2_body_resize(int w) {
    int x = 0;
    while (x <= w - 16) x += 16;
    while (x < w - 4) x += 4;
    return x;
}
inline int sse2_body_blur(int w) {
    int i = 0;
    while (i <= w - 16) i += 16;
    while (i <= w - 4) i += 4;
    return i;
}

// Host-side ctor tables (ORBextractor.cc:409-469) + blur taps.
struct HostTables {
    orbfe_params p;
    float scale[kMaxLevels], inv[kMaxLevels], sigma2[kMaxLevels], inv_sigma2[kMaxLevels];
    int nfeat[kMaxLevels];
    int umax[16];
    int taps[7];
};

// Everything that depends on the input size.
struct Plan {
    int w = 0, h = 0;
    Geo geo{};
    std::vector<CellDesc> cells;
    long long cell_cap_total = 0;
    std::vector<int> xtab, ytab;
    int xoff[kMaxLevels] = {}, yoff[kMaxLevels] = {};
    long long slab = 0;
    std::vector<uint32_t> bitems;  // blur_mfma_kernel work items (blur_items)
    struct Pyr {  // plan_pyramid
        struct Resize {  // resize_kernel: 128 x 32 tiles of one level
            int tiles_x[kMaxLevels] = {}, tiles[kMaxLevels] = {}, pitch[kMaxLevels] = {};
            size_t lds[kMaxLevels] = {};
        } rs;
        // resize2_kernel plans for the level pairs (l, l + 1): tile table offset (int4 units in tab)
        struct Resize2 {
            bool ok[kMaxLevels] = {};
            int tiles_x[kMaxLevels] = {}, tiles[kMaxLevels] = {}, off[kMaxLevels] = {};
            int pa[kMaxLevels] = {}, pb[kMaxLevels] = {}, bofs[kMaxLevels] = {};
            size_t lds[kMaxLevels] = {};
        } rs2;
        int tail_start = kMaxLevels;  // levels >= tail_start come from resize_tail_kernel
        // pyramid_kernel: column-group tables (all levels) then the band tables of the two band
        // plans (batches >= kTailMinFrames / smaller), in one device table of u32
        bool ok = false;
        bool use[2] = {false, false};  // per band plan: the band kernel is the faster path
        std::vector<uint32_t> tab;
        int gtab_off[kMaxLevels] = {};  // in uint4 units
        int band_off[2] = {}, nbands[2] = {}, bufb[2] = {}, ybuf[2] = {}, ymax[2] = {};
        int lp[kMaxLevels] = {};
        size_t lds[2] = {};
    } pyr;
    struct Fast {  // plan_fast: the dynamic-LDS carve of fast_kernel
        int roi_pitch = 0, roi_rows = 0, cand_max = 0;
        size_t lds = 0;
        // the pre-test's lane layouts, one per distinct (x0 & 3, candidate columns) of the
        // cells: kFastShapeStride uint2 each (fast_shape), and each cell's index into them
        std::vector<uint2> shapes;
        std::vector<int> cell_shape;
    } fast;
    struct Oct {  // plan_octree
        int ncap_max = 0, sort_cap = 0;
        int keys = 0;  // LDS key capacity of the oct-tree kernel
        size_t lds = 0;
    } oct;
};

// Environment switches: every getenv of the library is one of these three.
// Unset, or set to anything but "0".
inline bool env_on(const char* name) {
    const char* e = std::getenv(name);
    return !(e && std::strcmp(e, "0") == 0);
}
// Set to exactly `value`; without a value: set at all.
inline bool env_is(const char* name, const char* value = nullptr) {
    const char* e = std::getenv(name);
    return e && (!value || std::strcmp(e, value) == 0);
}
// The integer it holds (atoi's reading, or `base` 16 for masks), `dflt` when unset.  Read as
// unsigned, so a mask of any length keeps its low bits; a minus sign still negates.
inline long env_int(const char* name, long dflt, int base = 10) {
    const char* e = std::getenv(name);
    return e ? (long)std::strtoul(e, nullptr, base) : dflt;
}

}  // namespace orbfe
