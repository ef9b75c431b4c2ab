// orbfe_covis.hip — the covisibility graph of an orbfe_map: KeyFrame::UpdateConnections
// (KeyFrame.cc:1010-1100), AddConnection / UpdateBestCovisibles (:844-878), EraseConnection
// (:1295-1309) and the connection part of SetBadFlag (:1188-1199), DESIGN.md H27.
//
//   cov_count_kernel   one workgroup per batch keyframe: the counting loop (:1023-1041) into an LDS
//                      hash of keyframe slots, the counter compacted and sorted by order key, the
//                      lowest-key maximum and the entries the keyframe tells (count >= 15, or the
//                      maximum alone).  Run twice: for the sizes, then into rows of exactly that size
//   cov_merge_kernel   one workgroup per keyframe of the map, run twice: deciding (sizes, the
//                      capacity check, nothing written) and applying.  The tells addressed to the
//                      keyframe are looked up in the batch's counters, sorted by order key and
//                      merged into its row (its new counter, or its old weights); a changed weight
//                      re-sorts the whole row into the ordered list.  A one-entry tell is
//                      AddConnection / EraseConnection, no tell and a forced re-sort is
//                      UpdateBestCovisibles
//   cov_move_kernel / cov_set_ordered_kernel / cov_pos_kernel   rows that outgrow their region,
//                      the plain assignment of an ordered list, the batch positions
//
// The graph's columns, its row table (four lanes of cap ints per row) and pool are the store's
// (orbfe_map_store.hip): cov_ready() there makes them cover the map, CovDev is their view.
//
// A sequential batch has a closed form (tests/test_covis.py proves it against the literal loop on
// built and seeded maps): the counter C_i of keyframe i depends on points and
// observations only; i tells j when C_i[j] >= 15, or when no count of i reaches 15 and j is i's
// lowest-key maximum.  A batch keyframe j with a non-empty counter ends with C_j overridden by the
// tells of the keyframes after it; every other keyframe with its old weights overridden by all
// tells.  The ordered list is the full sort if a tell changed a weight, else the thresholded sort
// of C_j (or the old list).  Everything is integer; nothing depends on the order atomics land in:
// what an atomic appends is sorted by order key before it is read as an order.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "../../include/orbfe.h"
#include "orbfe_device.hpp"

namespace orbfe {

constexpr int kCovBlock = 1024;
constexpr int kCovMax = ORBFE_MAP_MAX_VOTED;   // entries of a counter / a weight map
constexpr int kCovHash = 2 * kCovMax;          // the counting hash: load <= 5/8 (see the guard)
constexpr int kCovTh = 15;                     // KeyFrame.cc:1051
constexpr int kCovTold = 1 << 30;              // flag on a counter entry: AddConnection is called
constexpr int kCovErase = -1;                  // weight of a tell that erases
constexpr int kCovRankBits = 12;               // a rank < 4096 under a weight <= 8192
static_assert(kCovMax == 1 << kCovRankBits, "a rank fills kCovRankBits");

enum { kCovOpBatch, kCovOpAdd, kCovOpErase, kCovOpBest, kCovOpEraseKf, kCovOpSetWeights };
enum { kCovErrCapacity = 1, kCovErrInternal = 2 };

// LDS bitonic sort of n_pad keys by all threads of the block.
template <class T>
__device__ __forceinline__ void cov_bitonic(T* k, int n_pad) {
    for (int size = 2; size <= n_pad; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = threadIdx.x; t < n_pad / 2; t += kCovBlock) {
                const int lo = 2 * t - (t & (stride - 1));
                const int hi = lo + stride;
                const bool up = ((lo & size) == 0);
                const T x = k[lo], y = k[hi];
                if ((x > y) == up) {
                    k[lo] = y;
                    k[hi] = x;
                }
            }
            __syncthreads();
        }
    }
}

// First position in the ascending keys k[0 .. n) that is not below `key`.
__device__ __forceinline__ int cov_lower_bound(const unsigned long long* k, int n, unsigned long long key) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (k[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// The same over keyframe slots s[0 .. n) that are in ascending order of their keys.
__device__ __forceinline__ int cov_lower_bound_slots(const int* s, int n, const unsigned long long* kf_key,
                                                     unsigned long long key) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (kf_key[s[mid]] < key) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// (slot, value) pairs rs / rv [0 .. n) in any order -> ss / sv in ascending key order, tk their
// keys.  n <= kCovMax; all LDS; every thread of the block calls it.
__device__ __forceinline__ void cov_sort_by_key(const unsigned long long* kf_key, int n, const int* rs,
                                                const int* rv, unsigned long long* tk, int* ss, int* sv) {
    int P = 1;
    while (P < n) P <<= 1;
    for (int t = threadIdx.x; t < P; t += kCovBlock) tk[t] = t < n ? kf_key[rs[t]] : ~0ull;
    __syncthreads();
    cov_bitonic(tk, P);
    for (int t = threadIdx.x; t < n; t += kCovBlock) {
        const int lo = cov_lower_bound(tk, n, kf_key[rs[t]]);
        ss[lo] = rs[t];
        sv[lo] = rv[t];
    }
    __syncthreads();
}

// sort(vPairs) then push_front (:1075-1082, :867-874): descending weight and, among equal weights,
// descending key.  ok[t] = 0 for an entry that is left out, else (weight << 12 | rank) + 1; after
// the call entry k of the list is cov_list_entry(ok, P, k).
__device__ __forceinline__ unsigned cov_list_key(int weight, int rank) {
    return (((unsigned)weight << kCovRankBits) | (unsigned)rank) + 1u;
}
__device__ __forceinline__ void cov_list_entry(const unsigned* ok, int P, int k, int& rank, int& weight) {
    const unsigned v = ok[P - 1 - k] - 1u;
    rank = (int)(v & (kCovMax - 1));
    weight = (int)(v >> kCovRankBits);
}

struct CovCountArgs {
    MapDev d;
    int n, fill;
    const int* batch;
    int* c_n;                // [n] the counter's size; kCovMax + 1: more than that
    const long long* c_off;  // [n] (fill) the row of keyframe p in c_slot / c_w
    int* c_slot;
    int* c_w;                // count | kCovTold
};

__global__ __launch_bounds__(kCovBlock) void cov_count_kernel(CovCountArgs a) {
    __shared__ unsigned long long big[kCovHash];  // the hash (slots, counts); then the sort keys and the order
    __shared__ int tl[kCovMax], tc[kCovMax];
    __shared__ int s_nd, s_np, s_any;
    __shared__ unsigned s_best;
    int* const hkey = reinterpret_cast<int*>(big);
    int* const hcnt = hkey + kCovHash;
    const MapDev& d = a.d;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int p = blockIdx.x;
    const int i = a.batch[p];
    for (int h = tid; h < kCovHash; h += kCovBlock) {
        hkey[h] = -1;
        hcnt[h] = 0;
    }
    if (tid == 0) s_nd = s_np = s_any = 0, s_best = 0;
    __syncthreads();
    const long long off = d.kf_mp_off[i];
    const int n_slots = min(d.kf_mp_n[i], kMapMaxSlots);
    for (int s = wave; s < n_slots; s += kCovBlock / 64) {  // :1023, as a vector: twice held counts twice
        const int mp = d.kf_mp[off + s];
        if (mp < 0 || mp >= d.n_mp) continue;               // :1027
        if (d.mp_bad[mp]) continue;                         // :1030
        const long long oo = d.mp_obs_off[mp];
        const int no = d.mp_obs_n[mp];
        for (int j = lane; j < no; j += 64) {
            const int kf = d.mp_obs[oo + j];
            if (kf < 0 || kf >= d.n_kf || kf == i) continue;  // :1037
            // more than kCovMax distinct keyframes is refused; until every thread has seen that,
            // each may insert one more, so the table holds at most kCovMax + 1 + kCovBlock of 8192
            if (*(volatile int*)&s_nd > kCovMax) break;
            unsigned h = ((unsigned)kf * 2654435761u) >> (32 - kCovRankBits - 1);
            for (;;) {
                int k = *(volatile int*)&hkey[h];
                if (k == -1) {
                    k = atomicCAS(&hkey[h], -1, kf);
                    if (k == -1) {
                        atomicAdd(&s_nd, 1);
                        k = kf;
                    }
                }
                if (k == kf) {
                    atomicAdd(&hcnt[h], 1);  // :1039
                    break;
                }
                h = (h + 1) & (kCovHash - 1);
            }
        }
    }
    __syncthreads();
    const int nd = s_nd;
    if (nd > kCovMax) {
        if (tid == 0) a.c_n[p] = kCovMax + 1;
        return;
    }
    if (!a.fill) {
        if (tid == 0) a.c_n[p] = nd;
        return;
    }
    for (int h = tid; h < kCovHash; h += kCovBlock)
        if (hkey[h] != -1) {
            const int q = atomicAdd(&s_np, 1);
            if (q < kCovMax) {
                tl[q] = hkey[h];
                tc[q] = hcnt[h];
            }
        }
    __syncthreads();
    if (nd == 0 || nd != a.c_n[p]) return;  // the sizes were taken from the same data
    // pointer order (:1055): the hash is dead, its memory holds the keys and the order
    unsigned long long* const keys = big;
    int* const order = reinterpret_cast<int*>(big + kCovMax);
    int P = 1;
    while (P < nd) P <<= 1;
    for (int t = tid; t < P; t += kCovBlock) keys[t] = t < nd ? d.kf_key[tl[t]] : ~0ull;
    __syncthreads();
    cov_bitonic(keys, P);
    for (int t = tid; t < nd; t += kCovBlock) {
        const int r = cov_lower_bound(keys, nd, d.kf_key[tl[t]]);
        order[r] = t;
        // nmax / pKFmax with `>` (:1057): the largest count at the lowest rank
        atomicMax(&s_best, ((unsigned)tc[t] << kCovRankBits) | (unsigned)(kCovMax - 1 - r));
        if (tc[t] >= kCovTh) s_any = 1;  // :1062
    }
    __syncthreads();
    const int best_r = kCovMax - 1 - (int)(s_best & (kCovMax - 1));
    const bool any = s_any != 0;
    const long long co = a.c_off[p];
    for (int r = tid; r < nd; r += kCovBlock) {
        const int t = order[r];
        const bool told = any ? tc[t] >= kCovTh : r == best_r;  // :1062-1073
        a.c_slot[co + r] = tl[t];
        a.c_w[co + r] = tc[t] | (told ? kCovTold : 0);
    }
}

struct CovMergeArgs {
    MapDev d;
    CovDev g;
    int op, apply, single;   // single >= 0: the one keyframe the launch is about
    // kCovOpBatch
    int n;
    const int* batch;
    const uint8_t* allow;    // [n] or NULL
    const int* c_n;
    const long long* c_off;
    const int* c_slot;
    const int* c_w;
    // the single-keyframe operations
    int slot, other, weight;
    int n_staged;
    const int* staged;       // kCovOpSetWeights: n_staged slots, then their weights
    int* parent_out;         // [n]
};

__global__ __launch_bounds__(kCovBlock) void cov_merge_kernel(CovMergeArgs a) {
    __shared__ unsigned long long tk[kCovMax];   // the tells' keys; then the list's sort keys
    __shared__ int ts[kCovMax], tw[kCovMax];     // the tells in key order
    __shared__ int bs[kCovMax], bw[kCovMax];     // the base row in key order
    __shared__ int ms[kCovMax], mw[kCovMax];     // sort buffer and raw tells; then the merged row
    __shared__ int tmp[kCovBlock / 64 + 1];
    __shared__ int s_nt, s_changed, s_cnt;
    const MapDev& d = a.d;
    const int tid = threadIdx.x;
    const int j = a.single >= 0 ? a.single : (int)blockIdx.x;
    int* const res = a.g.res + 3 * (size_t)j;
    if (a.apply && res[2] == 0) return;
    const unsigned long long key_j = d.kf_key[j];
    const int cap = a.g.cap[j];
    int* const w_slot = a.g.pool + a.g.off[j];
    int* const w_weight = w_slot + cap;
    int* const o_slot = w_slot + 2 * (size_t)cap;
    int* const o_weight = w_slot + 3 * (size_t)cap;
    const int old_nw = min(a.g.nw[j], min(cap, kCovMax)), old_no = a.g.no[j];
    if (tid == 0) s_nt = s_changed = s_cnt = 0;
    __syncthreads();

    if (a.op == kCovOpEraseKf && j == a.slot) {  // :1198-1199
        if (!a.apply) {
            if (tid == 0) res[0] = 0, res[1] = 0, res[2] = 1;
        } else {
            if (tid == 0) a.g.nw[j] = 0, a.g.no[j] = 0;
            if (tid < kMapNeigh) d.kf_neigh[j * kMapNeigh + tid] = -1;
        }
        return;
    }

    // ---- the base row: the keyframe's new counter (:1088), else its weights as they are
    const int pj = a.op == kCovOpBatch ? a.g.pos[j] : -1;
    const bool own = pj >= 0 && a.c_n[pj] > 0;  // an empty counter returns with nothing changed (:1044)
    int nb = 0, n_told = 0;
    if (own) {
        nb = min(a.c_n[pj], kCovMax);
        const long long co = a.c_off[pj];
        for (int t = tid; t < nb; t += kCovBlock) {
            bs[t] = a.c_slot[co + t];
            bw[t] = a.c_w[co + t];
        }
    } else if (a.op != kCovOpSetWeights) {
        nb = old_nw;
        for (int t = tid; t < nb; t += kCovBlock) {
            bs[t] = w_slot[t];
            bw[t] = w_weight[t];
        }
    }
    __syncthreads();
    if (own) {
        // the thresholded list (:1075-1090) and the parent (:1092-1097)
        unsigned* const ok = reinterpret_cast<unsigned*>(ms);
        int P = 1;
        while (P < nb) P <<= 1;
        for (int t = tid; t < P; t += kCovBlock) {
            const bool told = t < nb && (bw[t] & kCovTold);
            ok[t] = told ? cov_list_key(bw[t] & ~kCovTold, t) : 0u;
            if (told) atomicAdd(&s_cnt, 1);
        }
        __syncthreads();
        cov_bitonic(ok, P);
        n_told = s_cnt;
        if (a.apply) {
            if (n_told > cap) {
                if (tid == 0) atomicOr(&d.ctl[kCtlCallErr], kCovErrInternal);
                return;
            }
            for (int k = tid; k < n_told; k += kCovBlock) {
                int r, w;
                cov_list_entry(ok, P, k, r, w);
                o_slot[k] = bs[r];
                o_weight[k] = w;
                if (k < kMapNeigh) d.kf_neigh[j * kMapNeigh + k] = bs[r];
            }
            if (tid >= n_told && tid < kMapNeigh) d.kf_neigh[j * kMapNeigh + tid] = -1;
            if (tid == 0) {
                int parent = -1;
                if (a.g.first[j] && (!a.allow || a.allow[pj])) {
                    int r, w;
                    cov_list_entry(ok, P, 0, r, w);
                    parent = bs[r];  // the front: highest weight, highest key among ties
                    d.kf_parent[j] = parent;
                    a.g.first[j] = 0;
                }
                a.parent_out[pj] = parent;
            }
            __threadfence();  // a full re-sort below writes the same list and neighbours again
        }
        __syncthreads();
        for (int t = tid; t < nb; t += kCovBlock) bw[t] &= ~kCovTold;
        __syncthreads();
    }

    // ---- the tells addressed to this keyframe
    int* const rs = ms;
    int* const rv = mw;
    if (a.op == kCovOpBatch) {
        for (int p = tid; p < a.n; p += kCovBlock) {
            const int i = a.batch[p];
            if (i == j || (own && p < pj)) continue;  // what came before its own turn is overwritten
            const int cn = a.c_n[p];
            if (cn <= 0) continue;
            const long long co = a.c_off[p];
            const int lo = cov_lower_bound_slots(a.c_slot + co, cn, d.kf_key, key_j);
            if (lo >= cn || a.c_slot[co + lo] != j) continue;
            const int w = a.c_w[co + lo];
            if (!(w & kCovTold)) continue;
            const int q = atomicAdd(&s_nt, 1);
            if (q < kCovMax) {
                rs[q] = i;
                rv[q] = w & ~kCovTold;
            }
        }
    } else if (a.op == kCovOpAdd || a.op == kCovOpErase) {
        if (tid == 0) {
            rs[0] = a.other;
            rv[0] = a.op == kCovOpAdd ? a.weight : kCovErase;
            s_nt = 1;
        }
    } else if (a.op == kCovOpEraseKf) {
        if (tid == 0) {
            bool told = a.apply != 0;  // applying: decided already; the erased row is being cleared
            if (!a.apply) {            // :1188: every key of the erased keyframe's weight map
                const int sn = min(a.g.nw[a.slot], a.g.cap[a.slot]);
                const int* sp = a.g.pool + a.g.off[a.slot];
                const int lo = cov_lower_bound_slots(sp, sn, d.kf_key, key_j);
                told = lo < sn && sp[lo] == j;
            }
            if (told) {
                rs[0] = a.slot;
                rv[0] = kCovErase;
                s_nt = 1;
            }
        }
    } else if (a.op == kCovOpSetWeights) {
        const int ns = min(a.n_staged, kCovMax);
        for (int t = tid; t < ns; t += kCovBlock) {
            rs[t] = a.staged[t];
            rv[t] = a.staged[a.n_staged + t];
        }
        if (tid == 0) s_nt = ns;
    }
    __syncthreads();
    const int nt = s_nt;
    if (nt > kCovMax) {  // as many distinct keys: the weight map would pass kCovMax
        if (tid == 0) {
            atomicOr(&d.ctl[kCtlCallErr], kCovErrCapacity);
            res[0] = old_nw, res[1] = old_no, res[2] = 0;
        }
        return;
    }
    if (nt > 0) cov_sort_by_key(d.kf_key, nt, rs, rv, tk, ts, tw);

    // ---- AddConnection / EraseConnection of every tell against the base (:848-853, :1300-1304)
    for (int x = tid; x < nb; x += kCovBlock) {
        const int r = cov_lower_bound(tk, nt, d.kf_key[bs[x]]);
        if (r >= nt || ts[r] != bs[x]) continue;
        if (tw[r] == kCovErase) {
            bw[x] = -1;
            s_changed = 1;
        } else if (tw[r] != bw[x]) {
            bw[x] = tw[r];
            s_changed = 1;
        }
    }
    __syncthreads();
    for (int r = tid; r < nt; r += kCovBlock) {
        const int lo = cov_lower_bound_slots(bs, nb, d.kf_key, tk[r]);
        const bool present = lo < nb && bs[lo] == ts[r];
        if (present || tw[r] == kCovErase) tw[r] = -2;  // nothing to insert
        else s_changed = 1;
    }
    __syncthreads();
    // what stays of the base and what is inserted, each compacted in place (write index <= read index)
    int nb2 = 0, ni = 0;
    for (int c = 0; c < nb; c += kCovBlock) {
        const int x = c + tid;
        const bool keep = x < nb && bw[x] >= 0;
        const int s = x < nb ? bs[x] : 0, w = x < nb ? bw[x] : 0;
        int total;
        const int ex = block_exclusive_scan<kCovBlock>(keep ? 1 : 0, tmp, total);
        if (keep) {
            bs[nb2 + ex] = s;
            bw[nb2 + ex] = w;
        }
        nb2 += total;
        __syncthreads();
    }
    for (int c = 0; c < nt; c += kCovBlock) {
        const int r = c + tid;
        const bool keep = r < nt && tw[r] >= 0;
        const int s = r < nt ? ts[r] : 0, w = r < nt ? tw[r] : 0;
        const unsigned long long k = r < nt ? tk[r] : 0ull;
        int total;
        const int ex = block_exclusive_scan<kCovBlock>(keep ? 1 : 0, tmp, total);
        if (keep) {
            ts[ni + ex] = s;
            tw[ni + ex] = w;
            tk[ni + ex] = k;
        }
        ni += total;
        __syncthreads();
    }
    const int n_new = nb2 + ni;
    const bool resort = a.op == kCovOpBest || (s_changed && a.op != kCovOpSetWeights);
    const bool act = own || s_changed || resort || a.op == kCovOpSetWeights;
    if (n_new > kCovMax) {
        if (tid == 0) {
            atomicOr(&d.ctl[kCtlCallErr], kCovErrCapacity);
            res[0] = old_nw, res[1] = old_no, res[2] = 0;
        }
        return;
    }
    if (!a.apply) {
        if (tid == 0) {
            res[0] = act ? n_new : old_nw;
            res[1] = resort ? n_new : own ? n_told : old_no;
            res[2] = act ? 1 : 0;
        }
        return;
    }
    if (!act) return;
    if (n_new > cap) {
        if (tid == 0) atomicOr(&d.ctl[kCtlCallErr], kCovErrInternal);
        return;
    }
    // ---- the merged row, in key order; the raw tells in ms / mw are dead
    for (int x = tid; x < nb2; x += kCovBlock) {
        const int q = x + cov_lower_bound(tk, ni, d.kf_key[bs[x]]);
        ms[q] = bs[x];
        mw[q] = bw[x];
    }
    for (int r = tid; r < ni; r += kCovBlock) {
        const int q = r + cov_lower_bound_slots(bs, nb2, d.kf_key, tk[r]);
        ms[q] = ts[r];
        mw[q] = tw[r];
    }
    __syncthreads();
    for (int t = tid; t < n_new; t += kCovBlock) {
        w_slot[t] = ms[t];
        w_weight[t] = mw[t];
    }
    if (tid == 0) {
        a.g.nw[j] = n_new;
        if (own && !resort) a.g.no[j] = n_told;
    }
    if (!resort) return;
    // ---- UpdateBestCovisibles (:859-878): the whole row
    unsigned* const ok = reinterpret_cast<unsigned*>(tk);
    int P = 1;
    while (P < n_new) P <<= 1;
    for (int t = tid; t < P; t += kCovBlock) ok[t] = t < n_new ? cov_list_key(mw[t], t) : 0u;
    __syncthreads();
    cov_bitonic(ok, P);
    for (int k = tid; k < n_new; k += kCovBlock) {
        int r, w;
        cov_list_entry(ok, P, k, r, w);
        o_slot[k] = ms[r];
        o_weight[k] = w;
        if (k < kMapNeigh) d.kf_neigh[j * kMapNeigh + k] = ms[r];
    }
    if (tid >= n_new && tid < kMapNeigh) d.kf_neigh[j * kMapNeigh + tid] = -1;
    if (tid == 0) a.g.no[j] = n_new;
}

// A row that outgrew its region moves to a new one: both lists copied, then (off, cap).
struct CovMoveItem {
    long long new_off;
    int j, new_cap;
};

__global__ __launch_bounds__(256) void cov_move_kernel(const CovMoveItem* items, CovDev g) {
    int* const pool = g.pool;
    long long* const off = g.off;
    int* const cap = g.cap;
    const int* const nw = g.nw;
    const int* const no = g.no;
    const CovMoveItem it = items[blockIdx.x];
    const long long oo = off[it.j];
    const int oc = cap[it.j];
    const int n_w = min(nw[it.j], min(oc, it.new_cap)), n_o = min(no[it.j], min(oc, it.new_cap));
    for (int t = threadIdx.x; t < n_w; t += 256) {
        pool[it.new_off + t] = pool[oo + t];
        pool[it.new_off + it.new_cap + t] = pool[oo + oc + t];
    }
    for (int t = threadIdx.x; t < n_o; t += 256) {
        pool[it.new_off + 2ll * it.new_cap + t] = pool[oo + 2ll * oc + t];
        pool[it.new_off + 3ll * it.new_cap + t] = pool[oo + 3ll * oc + t];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        off[it.j] = it.new_off;
        cap[it.j] = it.new_cap;
    }
}

// mvpOrderedConnectedKeyFrames / mvOrderedWeights assigned: staged = n slots, then n weights.
__global__ __launch_bounds__(256) void cov_set_ordered_kernel(int j, int n, const int* staged, CovDev g,
                                                              int* kf_neigh) {
    int* const no = g.no;
    const int c = g.cap[j];
    if (n > c) return;
    int* const o_slot = g.pool + g.off[j] + 2ll * c;
    int* const o_weight = o_slot + c;
    for (int t = threadIdx.x; t < n; t += 256) {
        o_slot[t] = staged[t];
        o_weight[t] = staged[n + t];
    }
    if (threadIdx.x < kMapNeigh) kf_neigh[j * kMapNeigh + threadIdx.x] = threadIdx.x < n ? staged[threadIdx.x] : -1;
    if (threadIdx.x == 0) no[j] = n;
}

__global__ __launch_bounds__(256) void cov_pos_kernel(int n, const int* batch, int* pos) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p < n) pos[batch[p]] = p;
}

}  // namespace orbfe

namespace {

// Rows `need` = (keyframe, entries) get regions of at least that many entries, their contents
// kept: the table's plan, the pool's growth, one launch.
int cov_reserve(orbfe_map* m, const std::vector<std::pair<int, int>>& need) {
    std::vector<RowNeed> rows;
    for (const auto& x : need) rows.push_back({x.first, x.second, -1});
    const RowPlan plan = m->cov.plan(rows);
    if (plan.moves.empty()) return ORBFE_OK;
    std::vector<CovMoveItem> items;
    for (const RowMove& v : plan.moves) items.push_back({v.new_off, v.row, v.new_cap});
    int st;
    if ((st = store_grow_pool(m, m->cov_pool, sizeof(int), m->cov.used, plan.alloc, kFillZero))) return st;
    m->cov.commit(plan);
    CovMoveItem* d_items;
    if ((st = store_borrow(m, kStageItems, items.size(), d_items))) return st;
    ORBFE_HIP(hipMemcpyAsync(d_items, items.data(), sizeof(CovMoveItem) * items.size(), hipMemcpyHostToDevice,
                             m->stream));
    hipLaunchKernelGGL(cov_move_kernel, dim3((unsigned)items.size()), dim3(256), 0, m->stream, d_items, cov_dev(m));
    ORBFE_HIP(hipGetLastError());
    ORBFE_HIP(hipStreamSynchronize(m->stream));
    return ORBFE_OK;
}

CovMergeArgs cov_args(int op, int single) {
    CovMergeArgs a{};
    a.op = op;
    a.single = single;
    a.slot = single;
    return a;
}

// Decides (sizes and the capacity check, nothing written), grows the rows that need it, applies.
// single >= 0: one workgroup for that keyframe; else one per keyframe of the map.  The views are
// taken ahead of each launch: the rows' growth between the two may move the graph's pool.
int cov_run(orbfe_map* m, CovMergeArgs a) {
    const int grid = a.single >= 0 ? 1 : m->n_kf;
    if (grid <= 0) return ORBFE_OK;
    const int first = a.single >= 0 ? a.single : 0;
    std::vector<int> res(3 * (size_t)grid);
    int st, err = 0;
    if ((st = store_clear_err(m))) return st;
    a.apply = 0;
    a.d = m->dev();
    a.g = cov_dev(m);
    a.parent_out = m->pout.as<int>();
    hipLaunchKernelGGL(cov_merge_kernel, dim3(grid), dim3(kCovBlock), 0, m->stream, a);
    ORBFE_HIP(hipGetLastError());
    ORBFE_HIP(hipMemcpyAsync(res.data(), a.g.res + 3 * (size_t)first, sizeof(int) * res.size(),
                             hipMemcpyDeviceToHost, m->stream));
    if ((st = store_read_err(m, err))) return st;
    if (err & kCovErrCapacity) return ORBFE_ERR_CAPACITY;
    if (err) return ORBFE_ERR_HIP;
    std::vector<std::pair<int, int>> need;
    for (int g = 0; g < grid; ++g)
        if (res[3 * g + 2]) need.push_back({first + g, std::max(res[3 * g], res[3 * g + 1])});
    if (need.empty()) return ORBFE_OK;
    if ((st = cov_reserve(m, need))) return st;
    a.apply = 1;
    a.d = m->dev();
    a.g = cov_dev(m);
    hipLaunchKernelGGL(cov_merge_kernel, dim3(grid), dim3(kCovBlock), 0, m->stream, a);
    ORBFE_HIP(hipGetLastError());
    if ((st = store_read_err(m, err))) return st;
    if (err) return ORBFE_ERR_HIP;
    for (int g = 0; g < grid; ++g)
        if (res[3 * g + 2]) {
            m->h_nw[first + g] = res[3 * g];
            m->h_no[first + g] = res[3 * g + 1];
        }
    return ORBFE_OK;
}

// n slots then n weights staged on the device.
int cov_stage(orbfe_map* m, int n, const int32_t* slots, const int32_t* weights, int*& staged) {
    int st;
    if ((st = store_borrow(m, kStageVals, 2 * (size_t)n, staged))) return st;
    if (n) {
        ORBFE_HIP(hipMemcpyAsync(staged, slots, sizeof(int) * (size_t)n, hipMemcpyHostToDevice, m->stream));
        ORBFE_HIP(hipMemcpyAsync(staged + n, weights, sizeof(int) * (size_t)n, hipMemcpyHostToDevice, m->stream));
    }
    return ORBFE_OK;
}

// AddChild (KeyFrame.cc:1102-1106) of every assigned (child, parent): a set union per parent,
// read from and written to the children rows in one copy and one launch.
int cov_add_children(orbfe_map* m, int n, const int32_t* kf_slots, const int* parents) {
    std::vector<std::pair<int, int>> pc;  // (parent, child)
    for (int i = 0; i < n; ++i)
        if (parents[i] >= 0) pc.push_back({parents[i], kf_slots[i]});
    if (pc.empty()) return ORBFE_OK;
    std::sort(pc.begin(), pc.end());
    const RowTable& r = m->kf_ch;
    std::vector<int> pool((size_t)r.used);
    if (r.used) {
        ORBFE_HIP(hipMemcpyAsync(pool.data(), m->kf_ch_pool.buf.p, sizeof(int) * (size_t)r.used,
                                 hipMemcpyDeviceToHost, m->stream));
        ORBFE_HIP(hipStreamSynchronize(m->stream));
    }
    std::vector<std::vector<int>> rows;
    std::vector<int> who;
    for (size_t b = 0; b < pc.size();) {
        const int p = pc[b].first;
        std::vector<int> ch;
        if (r.length(p)) ch.assign(pool.begin() + r.off[p], pool.begin() + r.off[p] + r.len[p]);
        for (; b < pc.size() && pc[b].first == p; ++b) ch.push_back(pc[b].second);
        std::sort(ch.begin(), ch.end(), [&](int x, int y) { return m->h_key[x] < m->h_key[y]; });
        ch.erase(std::unique(ch.begin(), ch.end()), ch.end());
        rows.push_back(std::move(ch));
        who.push_back(p);
    }
    std::vector<MapRowWrite> w;
    for (size_t k = 0; k < rows.size(); ++k)
        w.push_back({who[k], 0, (int)rows[k].size(), (int)rows[k].size(), rows[k].data(), nullptr});
    return map_put_kf_ch(m, w);
}

int cov_get_row(orbfe_map* m, int slot, bool ordered, int32_t* kf_slots, int32_t* weights, int cap, int32_t* n) {
    if (!m || !n || cap < 0 || (cap && !kf_slots)) return ORBFE_ERR_ARG;
    if (!m->kf_ok(slot)) return ORBFE_ERR_ARG;
    return map_guarded(m, [&]() {
        int st;
        if ((st = cov_ready(m))) return st;
        const RowTable& r = m->cov;
        *n = ordered ? m->h_no[slot] : m->h_nw[slot];
        if (*n > cap) return (int)ORBFE_ERR_CAPACITY;
        if (!*n) return (int)ORBFE_OK;
        const int* row = m->cov_pool.buf.as<int>() + r.off[slot] + (ordered ? 2ll * r.cap[slot] : 0ll);
        ORBFE_HIP(hipMemcpyAsync(kf_slots, row, sizeof(int) * (size_t)*n, hipMemcpyDeviceToHost, m->stream));
        if (weights)
            ORBFE_HIP(hipMemcpyAsync(weights, row + r.cap[slot], sizeof(int) * (size_t)*n,
                                     hipMemcpyDeviceToHost, m->stream));
        ORBFE_HIP(hipStreamSynchronize(m->stream));
        return (int)ORBFE_OK;
    });
}

// One of the single-keyframe operations on `slot`.
int cov_single(orbfe_map* m, int op, int slot, int other, int weight) {
    return map_guarded(m, [&]() {
        int st;
        if ((st = cov_ready(m))) return st;
        CovMergeArgs a = cov_args(op, op == kCovOpEraseKf ? -1 : slot);
        a.slot = slot;
        a.other = other;
        a.weight = weight;
        return cov_run(m, a);
    });
}

}  // namespace

extern "C" {

int orbfe_map_update_connections(orbfe_map* m, int n, const int32_t* kf_slots, const uint8_t* allow_parent,
                                 int32_t* parent_out, int32_t* n_ordered_out) {
    if (!m || n < 0 || (n && !kf_slots)) return ORBFE_ERR_ARG;
    {
        std::vector<int> s(kf_slots, kf_slots + n);
        std::sort(s.begin(), s.end());
        for (int i = 0; i < n; ++i)
            if (!m->kf_ok(s[i]) || (i && s[i] == s[i - 1])) return ORBFE_ERR_ARG;
    }
    if (!n) return ORBFE_OK;
    return map_guarded(m, [&]() {
        int st;
        if ((st = cov_ready(m))) return st;
        const size_t ni = sizeof(int) * (size_t)n;
        if ((st = m->batch.ensure(ni))) return st;
        if ((st = m->c_n.ensure(ni))) return st;
        if ((st = m->c_off.ensure(8 * (size_t)n))) return st;
        if ((st = m->pout.ensure(ni))) return st;
        if ((st = m->allow.ensure((size_t)n))) return st;
        ORBFE_HIP(hipMemcpyAsync(m->batch.p, kf_slots, ni, hipMemcpyHostToDevice, m->stream));
        if (allow_parent) ORBFE_HIP(hipMemcpyAsync(m->allow.p, allow_parent, (size_t)n, hipMemcpyHostToDevice, m->stream));
        ORBFE_HIP(hipMemsetAsync(m->at<int>(kColCovPos), 0xff, sizeof(int) * (size_t)m->n_kf, m->stream));
        ORBFE_HIP(hipMemsetAsync(m->pout.p, 0xff, ni, m->stream));
        hipLaunchKernelGGL(cov_pos_kernel, dim3((n + 255) / 256), dim3(256), 0, m->stream, n,
                           m->batch.as<int>(), m->at<int>(kColCovPos));
        // the counters: their sizes, then rows of exactly those sizes
        CovCountArgs k{};
        k.d = m->dev();
        k.n = n;
        k.batch = m->batch.as<int>();
        k.c_n = m->c_n.as<int>();
        hipLaunchKernelGGL(cov_count_kernel, dim3(n), dim3(kCovBlock), 0, m->stream, k);
        ORBFE_HIP(hipGetLastError());
        std::vector<int> cn((size_t)n);
        ORBFE_HIP(hipMemcpyAsync(cn.data(), m->c_n.p, ni, hipMemcpyDeviceToHost, m->stream));
        ORBFE_HIP(hipStreamSynchronize(m->stream));
        std::vector<long long> coff((size_t)n);
        long long total = 0;
        for (int i = 0; i < n; ++i) {
            if (cn[i] > kCovMax) return (int)ORBFE_ERR_CAPACITY;
            coff[i] = total;
            total += cn[i];
        }
        if ((st = m->c_slot.ensure(sizeof(int) * (size_t)std::max<long long>(total, 1)))) return st;
        if ((st = m->c_w.ensure(sizeof(int) * (size_t)std::max<long long>(total, 1)))) return st;
        ORBFE_HIP(hipMemcpyAsync(m->c_off.p, coff.data(), 8 * (size_t)n, hipMemcpyHostToDevice, m->stream));
        k.fill = 1;
        k.c_off = m->c_off.as<long long>();
        k.c_slot = m->c_slot.as<int>();
        k.c_w = m->c_w.as<int>();
        hipLaunchKernelGGL(cov_count_kernel, dim3(n), dim3(kCovBlock), 0, m->stream, k);
        ORBFE_HIP(hipGetLastError());
        CovMergeArgs a = cov_args(kCovOpBatch, -1);
        a.n = n;
        a.batch = k.batch;
        a.allow = allow_parent ? m->allow.as<uint8_t>() : nullptr;
        a.c_n = k.c_n;
        a.c_off = k.c_off;
        a.c_slot = k.c_slot;
        a.c_w = k.c_w;
        if ((st = cov_run(m, a))) return st;
        std::vector<int> par((size_t)n);
        ORBFE_HIP(hipMemcpyAsync(par.data(), m->pout.p, ni, hipMemcpyDeviceToHost, m->stream));
        ORBFE_HIP(hipStreamSynchronize(m->stream));
        if ((st = cov_add_children(m, n, kf_slots, par.data()))) return st;
        for (int i = 0; i < n; ++i) {
            if (parent_out) parent_out[i] = par[i];
            if (n_ordered_out) n_ordered_out[i] = m->h_no[kf_slots[i]];
        }
        return (int)ORBFE_OK;
    });
}

int orbfe_map_add_connection(orbfe_map* m, int slot, int other, int weight) {
    if (!m || !m->kf_ok(slot) || !m->kf_ok(other) || weight < 0 || weight > kMapMaxSlots) return ORBFE_ERR_ARG;
    return cov_single(m, kCovOpAdd, slot, other, weight);
}

int orbfe_map_erase_connection(orbfe_map* m, int slot, int other) {
    if (!m || !m->kf_ok(slot) || !m->kf_ok(other)) return ORBFE_ERR_ARG;
    return cov_single(m, kCovOpErase, slot, other, 0);
}

int orbfe_map_update_best_covisibles(orbfe_map* m, int slot) {
    if (!m || !m->kf_ok(slot)) return ORBFE_ERR_ARG;
    return cov_single(m, kCovOpBest, slot, -1, 0);
}

int orbfe_map_erase_keyframe_connections(orbfe_map* m, int slot) {
    if (!m || !m->kf_ok(slot)) return ORBFE_ERR_ARG;
    return cov_single(m, kCovOpEraseKf, slot, -1, 0);
}

static int cov_check_list(const orbfe_map* m, int n, const int32_t* kf_slots, const int32_t* weights,
                          bool distinct) {
    if (n < 0 || n > kCovMax || (n && (!kf_slots || !weights))) return ORBFE_ERR_ARG;
    for (int i = 0; i < n; ++i)
        if (!m->kf_ok(kf_slots[i]) || weights[i] < 0 || weights[i] > kMapMaxSlots) return ORBFE_ERR_ARG;
    if (distinct) {
        std::vector<int> s(kf_slots, kf_slots + n);
        std::sort(s.begin(), s.end());
        if (std::adjacent_find(s.begin(), s.end()) != s.end()) return ORBFE_ERR_ARG;
    }
    return ORBFE_OK;
}

int orbfe_map_set_connections(orbfe_map* m, int slot, int n, const int32_t* kf_slots, const int32_t* weights) {
    if (!m || !m->kf_ok(slot) || cov_check_list(m, n, kf_slots, weights, true)) return ORBFE_ERR_ARG;
    return map_guarded(m, [&]() {
        int st;
        if ((st = cov_ready(m))) return st;
        CovMergeArgs a = cov_args(kCovOpSetWeights, slot);
        int* staged;
        if ((st = cov_stage(m, n, kf_slots, weights, staged))) return st;
        a.n_staged = n;
        a.staged = staged;
        return cov_run(m, a);
    });
}

int orbfe_map_set_ordered_connections(orbfe_map* m, int slot, int n, const int32_t* kf_slots,
                                      const int32_t* weights) {
    if (!m || !m->kf_ok(slot) || cov_check_list(m, n, kf_slots, weights, false)) return ORBFE_ERR_ARG;
    return map_guarded(m, [&]() {
        int st;
        if ((st = cov_ready(m))) return st;
        int* staged;
        if ((st = cov_stage(m, n, kf_slots, weights, staged))) return st;
        if ((st = cov_reserve(m, {{slot, n}}))) return st;
        hipLaunchKernelGGL(cov_set_ordered_kernel, dim3(1), dim3(256), 0, m->stream, slot, n, staged, cov_dev(m),
                           m->at<int>(kColKfNeigh));
        ORBFE_HIP(hipGetLastError());
        ORBFE_HIP(hipStreamSynchronize(m->stream));
        m->h_no[slot] = n;
        return (int)ORBFE_OK;
    });
}

int orbfe_map_set_first_connection(orbfe_map* m, int slot, int flag) {
    if (!m || !m->kf_ok(slot)) return ORBFE_ERR_ARG;
    return map_guarded(m, [&]() {
        int st;
        if ((st = cov_ready(m))) return st;
        const int32_t s = slot;
        return store_set<uint8_t>(m, m->at<uint8_t>(kColCovFirst), 1, &s, nullptr, flag ? 1 : 0);
    });
}

int orbfe_map_get_connections(orbfe_map* m, int slot, int32_t* kf_slots, int32_t* weights, int cap, int32_t* n) {
    return cov_get_row(m, slot, false, kf_slots, weights, cap, n);
}

int orbfe_map_get_ordered_connections(orbfe_map* m, int slot, int32_t* kf_slots, int32_t* weights, int cap,
                                      int32_t* n) {
    return cov_get_row(m, slot, true, kf_slots, weights, cap, n);
}

int orbfe_map_get_spanning_tree(orbfe_map* m, int slot, int32_t* parent, int32_t* first_connection,
                                int32_t* child_slots, int cap, int32_t* n_children) {
    if (!m || !n_children || cap < 0 || (cap && !child_slots) || !m->kf_ok(slot)) return ORBFE_ERR_ARG;
    return map_guarded(m, [&]() {
        int st;
        if ((st = cov_ready(m))) return st;
        const RowTable& r = m->kf_ch;
        *n_children = r.length(slot);
        if (*n_children > cap) return (int)ORBFE_ERR_CAPACITY;
        int p = -1;
        uint8_t f = 0;
        ORBFE_HIP(hipMemcpyAsync(&p, m->at<int>(kColKfParent) + slot, sizeof(int), hipMemcpyDeviceToHost, m->stream));
        ORBFE_HIP(hipMemcpyAsync(&f, m->at<uint8_t>(kColCovFirst) + slot, 1, hipMemcpyDeviceToHost, m->stream));
        if (*n_children)
            ORBFE_HIP(hipMemcpyAsync(child_slots, m->kf_ch_pool.buf.as<int>() + r.off[slot],
                                     sizeof(int) * (size_t)*n_children, hipMemcpyDeviceToHost, m->stream));
        ORBFE_HIP(hipStreamSynchronize(m->stream));
        if (parent) *parent = p;
        if (first_connection) *first_connection = f;
        return (int)ORBFE_OK;
    });
}

}  // extern "C"
