// orbfe_kfdb.hip — ORBVocabulary::score and the keyframe database (KeyFrameDatabase.cc:115-389):
// the BoW similarity scores and the loop / relocalisation candidate lists, so that the chain
// BoW transform -> candidates -> SearchByBoW stays on the device.
//
//   bow_score_pairs_kernel  one wave per (slot, slot) pair: ORBVocabulary::score
//   kfdb_score_kernel       one launch per query, one wave per database slot: common-word count,
//                           first common word and the double score; the last workgroup to finish
//                           runs the whole tail of DetectLoopCandidates /
//                           DetectRelocalizationCandidates (state update, thresholds, the sort
//                           into the inverted-file walk's order, covisibility accumulation,
//                           retain test, duplicates) and writes the done word the host waits on
//   kfdb_slot_kernel / kfdb_erase_kernel / kfdb_covis_kernel / kfdb_scores_kernel
//                           KeyFrameDatabase::add / erase and the per-keyframe state
//
// The reference walks an inverted file (word -> list of keyframes in add order).  The walk's
// first-encounter order is the sort key (first common word, add sequence), so a dense pass over
// the slots plus that key reproduces every list of the reference without an inverted file.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/orbfe.h"
#include "orbfe_device.hpp"

namespace orbfe {

constexpr int kKfdbBlock = 1024;          // 16 waves = 16 slots per workgroup; the tail's width
constexpr int kKfdbMaxWords = 4096;       // words per BowVector (query ids staged in 16 KB of LDS)
constexpr int kKfdbMaxEntries = 4096;     // scored keyframes the tail sorts in LDS
constexpr int kKfdbNeigh = 10;            // GetBestCovisibilityKeyFrames(10)
constexpr int kBowScoreUnroll = 8;        // 64-word chunks a wave has in flight

// Lane `lane` (wave-uniform) of a double.
__device__ __forceinline__ double lane_double(double x, int lane) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(x), lane);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(x), lane);
    return __hiloint2double(hi, lo);
}

// ORBVocabulary::score(v1, v2) (TemplatedVocabulary.h -> ScoringObject.cpp:23-311) by one wave.
// v1 = (qi, qv, nq), v2 = (ki, kv, nk), word ids strictly ascending.  The lanes take v2's words
// and binary-search v1; the common words' terms are added to one double accumulator in ascending
// word order by a serial walk over the ballot bits (the sum is not associative).  `fused`: the
// reference's -O3 -march=native build contracts `score += vi * wi` of the L2 and dot-product
// loops (:91, :290) into fma(vi, wi, score).  count = the common words, first =
// the smallest common word id (-1: none).  Every lane returns the same values.
__device__ __forceinline__ double wave_bow_score(const int* qi, const double* qv, int nq,
                                                 const int* ki, const double* kv, int nk,
                                                 int scoring, bool fused, int& count, int& first) {
    const int lane = threadIdx.x & 63;
    double score = 0.0;
    count = 0;
    first = -1;
    // kBowScoreUnroll chunks of 64 words at a time: their ids, their searches (in lockstep, a
    // fixed number of halvings) and the matched values are batches of independent loads, so a
    // wave waits for memory three times per 512 words rather than three times per 64 (measured:
    // profiles/kfdb/README.md)
    const int steps = nq > 0 ? 32 - __clz(nq) : 0;
    for (int base = 0; base < nk; base += 64 * kBowScoreUnroll) {
        int w[kBowScoreUnroll], lo[kBowScoreUnroll], hi[kBowScoreUnroll];
#pragma unroll
        for (int u = 0; u < kBowScoreUnroll; ++u) {
            const int i = base + 64 * u + lane;
            w[u] = i < nk ? ki[i] : -1;
            lo[u] = 0;
            hi[u] = i < nk ? nq : 0;
        }
        for (int s = 0; s < steps; ++s) {
#pragma unroll
            for (int u = 0; u < kBowScoreUnroll; ++u)
                if (lo[u] < hi[u]) {
                    const int mid = (lo[u] + hi[u]) >> 1;
                    if (qi[mid] < w[u]) lo[u] = mid + 1;
                    else hi[u] = mid;
                }
        }
        double vi[kBowScoreUnroll], wi[kBowScoreUnroll];
        bool hit[kBowScoreUnroll];
#pragma unroll
        for (int u = 0; u < kBowScoreUnroll; ++u) {
            const int i = base + 64 * u + lane;
            hit[u] = i < nk && lo[u] < nq && qi[lo[u]] == w[u];
            vi[u] = hit[u] ? qv[lo[u]] : 0.0;
            wi[u] = hit[u] ? kv[i] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < kBowScoreUnroll; ++u) {
            const unsigned long long m = __ballot(hit[u]);
            if (!m) continue;
            if (first < 0) first = __builtin_amdgcn_readlane(w[u], __ffsll((long long)m) - 1);
            count += __popcll(m);
            double t = 0.0;
            bool use = hit[u];
            if (use) {
                switch (scoring) {
                    case 0: t = fabs(vi[u] - wi[u]) - fabs(vi[u]) - fabs(wi[u]); break;   // :41
                    case 2:                                                               // :148
                        use = vi[u] + wi[u] != 0.0;
                        if (use) t = vi[u] * wi[u] / (vi[u] + wi[u]);
                        break;
                    case 4: t = sqrt(vi[u] * wi[u]); break;                               // :245
                    default: t = vi[u] * wi[u]; break;                                    // :91, :290
                }
            }
            unsigned long long mt = __ballot(use);
            while (mt) {
                const int b = __ffsll((long long)mt) - 1;
                mt &= mt - 1;
                if (fused) score = fma(lane_double(vi[u], b), lane_double(wi[u], b), score);
                else score += lane_double(t, b);
            }
        }
    }
    switch (scoring) {
        case 0: score = -score / 2.0; break;                                      // :65
        case 1: score = score >= 1 ? 1.0 : 1.0 - sqrt(1.0 - score); break;        // :114-117
        case 2: score = 2. * score; break;                                        // :167
        default: break;
    }
    return score;
}

struct ScorePairsArgs {
    int n_pairs, cap, scoring, fused;
    const int* pair_a;
    const int* pair_b;
    const int* ids;
    const double* vals;
    const int* nw;
    double* out;
};

__global__ __launch_bounds__(kKfdbBlock) void bow_score_pairs_kernel(ScorePairsArgs a) {
    const int p = blockIdx.x * (kKfdbBlock / 64) + (threadIdx.x >> 6);
    if (p >= a.n_pairs) return;
    const int sa = a.pair_a[p], sb = a.pair_b[p];
    if (sa < 0 || sb < 0) {
        if ((threadIdx.x & 63) == 0) a.out[p] = 0.0;
        return;
    }
    const int na = min(max(a.nw[sa], 0), a.cap), nb = min(max(a.nw[sb], 0), a.cap);
    int count, first;
    const double s = wave_bow_score(a.ids + (size_t)sa * a.cap, a.vals + (size_t)sa * a.cap, na,
                                    a.ids + (size_t)sb * a.cap, a.vals + (size_t)sb * a.cap, nb,
                                    a.scoring, a.fused != 0, count, first);
    if ((threadIdx.x & 63) == 0) a.out[p] = s;
}

// Device storage of the database: slot s holds a BowVector in the BoW-transform layout (word ids
// and values at s*cap, nw[s]; nw = 0 for a free slot), its add sequence number, its covisibility
// list (kKfdbNeigh slots, -1 = none) and the six state fields of KeyFrame.h:166-171.
struct KfdbDev {
    int cap, nslots;  // nslots: the high-water mark of used slots
    int* ids;
    double* vals;
    int* nw;
    unsigned* seq;
    int* neigh;
    orbfe_kfdb_state* st;
    // per-query scratch
    int* cnt;
    int* firstw;
    double* dscore;
    unsigned* conn;            // stamped with the call's epoch for connected slots
    int* first_e;
    unsigned long long* ekey;  // the compacted entries' keys and slots
    int* eslot;
};

struct KfdbQuery {
    KfdbDev d;
    int loop;                  // 1: DetectLoopCandidates, 0: DetectRelocalizationCandidates
    unsigned long long qid;    // pKF->mnId / F->mnId
    const int* q_ids;
    const double* q_vals;
    const int* q_nw;
    int n_conn;
    const int* conn_slots;
    unsigned epoch;
    float min_score;
    int scoring, fused;
    int* cand;
    int cand_cap;
    int* result;               // device-mapped pinned: n_cand, status, done
    int* counter;
};

__global__ __launch_bounds__(kKfdbBlock) void kfdb_score_kernel(KfdbQuery a) {
    // 48 KB, reused: the query's word ids (score pass); the sort keys (32 KB) and the sorted
    // slots (16 KB); the accumulated scores and best keyframes over the keys
    __shared__ unsigned long long lds[kKfdbMaxEntries + kKfdbMaxEntries / 2];
    __shared__ int tmp[kKfdbBlock / 64 + 1];
    __shared__ float s_best[kKfdbBlock];
    __shared__ int s_max, s_cnt, s_h18;
    const int tid = threadIdx.x;
    const KfdbDev& d = a.d;
    const int N = d.nslots;
    {
        int* qi = reinterpret_cast<int*>(lds);
        const int nq = min(max(*a.q_nw, 0), min(d.cap, kKfdbMaxWords));
        for (int i = tid; i < nq; i += kKfdbBlock) qi[i] = a.q_ids[i];
        __syncthreads();
        const int s = blockIdx.x * (kKfdbBlock / 64) + (tid >> 6);
        if (s < N) {
            const int nk = min(max(d.nw[s], 0), d.cap);
            int count, first;
            const double sc = wave_bow_score(qi, a.q_vals, nq, d.ids + (size_t)s * d.cap,
                                             d.vals + (size_t)s * d.cap, nk, a.scoring,
                                             a.fused != 0, count, first);
            if ((tid & 63) == 0) {
                d.cnt[s] = count;
                d.firstw[s] = first;
                d.dscore[s] = sc;
            }
        }
    }
    if (!last_workgroup(a.counter)) return;

    // ---- the tail (KeyFrameDatabase.cc:161-271 / 282-388), one workgroup
    {   // a query vector the score pass cannot have read as a BowVector (a count outside
        // [0, cap], ids not strictly ascending) is refused before any state is touched
        const int nq = *a.q_nw;
        int bad = nq < 0 || nq > min(d.cap, kKfdbMaxWords);
        if (!bad)
            for (int i = tid + 1; i < nq; i += kKfdbBlock)
                if (a.q_ids[i - 1] >= a.q_ids[i]) bad = 1;
        if (__syncthreads_or(bad)) {
            if (tid == 0) {
                *a.counter = 0;
                a.result[0] = 0;
                a.result[1] = ORBFE_ERR_ARG;
                __hip_atomic_store(&a.result[2], 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
            }
            return;
        }
    }
    if (tid == 0) {
        s_max = 0;
        s_cnt = 0;
        s_h18 = 0;
    }
    if (a.loop)  // spConnectedKeyFrames (:153)
        for (int i = tid; i < a.n_conn; i += kKfdbBlock) {
            const int c = a.conn_slots[i];
            if (c >= 0 && c < N) d.conn[c] = a.epoch;
        }
    __syncthreads();
    // the walk's effect on each sharing keyframe (:161-179 / :282-302): c encounters
    for (int s = tid; s < N; s += kKfdbBlock) {
        d.first_e[s] = INT_MAX;
        const int c = d.cnt[s];
        if (c <= 0) continue;
        orbfe_kfdb_state& st = d.st[s];
        uint64_t& query = a.loop ? st.loop_query : st.reloc_query;
        int32_t& words = a.loop ? st.loop_words : st.reloc_words;
        int listed = 0;
        if (query == a.qid) {
            words += c;          // H19: not reset, not listed again
        } else if (a.loop && d.conn[s] == a.epoch) {
            words = 1;           // reset on every encounter (:170), then ++ (:177)
        } else {
            query = a.qid;
            words = c;
            listed = 1;
            atomicMax(&s_max, c);  // maxCommonWords (:188-193)
        }
        d.cnt[s] = listed ? c : 0;
    }
    __syncthreads();
    const int min_common = (int)(s_max * 0.8f);  // :195, :315
    int status = ORBFE_OK, n_cand = 0;
    // scores of the keyframes that share enough words (:200-214 / :322-333)
    unsigned long long* keys = lds;
    for (int s = tid; s < N; s += kKfdbBlock) {
        const int c = d.cnt[s];
        if (c <= 0 || !(c > min_common)) continue;
        const float si = (float)d.dscore[s];
        orbfe_kfdb_state& st = d.st[s];
        if (a.loop) {
            st.loop_score = si;
            st.scores_set |= 1;
        } else {
            st.reloc_score = si;
            st.scores_set |= 2;
        }
        if (a.loop && !(si >= a.min_score)) continue;
        const int pos = atomicAdd(&s_cnt, 1);
        if (pos < kKfdbMaxEntries) {
            const unsigned long long key = ((unsigned long long)(unsigned)d.firstw[s] << 32) | d.seq[s];
            keys[pos] = key;
            d.ekey[pos] = key;
            d.eslot[pos] = s;
        }
    }
    __syncthreads();
    const int E = s_cnt;
    if (E > kKfdbMaxEntries) {
        status = ORBFE_ERR_CAPACITY;
        n_cand = E;
    } else if (E > 0) {
        // lScoreAndMatch in list order: sorted by (first common word, add sequence)
        int P = 1;
        while (P < E) P <<= 1;
        for (int t = E + tid; t < P; t += kKfdbBlock) keys[t] = ~0ull;
        __syncthreads();
        bitonic_sort_u64(keys, P);
        int* order = reinterpret_cast<int*>(lds + kKfdbMaxEntries);
        for (int i = tid; i < E; i += kKfdbBlock) {
            const unsigned long long key = d.ekey[i];
            int lo = 0, hi = E;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (keys[mid] < key) lo = mid + 1;
                else hi = mid;
            }
            order[lo] = d.eslot[i];
        }
        __syncthreads();
        // covisibility accumulation (:223-248 / :342-367), one thread per entry
        float* acc = reinterpret_cast<float*>(lds);
        int* best = reinterpret_cast<int*>(lds) + kKfdbMaxEntries;
        float lmax = a.loop ? a.min_score : 0.f;  // bestAccScore (:220, :339)
        for (int e = tid; e < E; e += kKfdbBlock) {
            const int s = order[e];
            const float own = a.loop ? d.st[s].loop_score : d.st[s].reloc_score;
            float best_score = own, acc_score = own;
            int bk = s;
            // the ten neighbours' ids, then their states, as two batches of independent loads
            // (one workgroup does this alone: a chain of dependent loads per neighbour is serial)
            int nb[kKfdbNeigh], set[kKfdbNeigh];
            bool ok[kKfdbNeigh];
            float sc[kKfdbNeigh];
#pragma unroll
            for (int j = 0; j < kKfdbNeigh; ++j) nb[j] = d.neigh[s * kKfdbNeigh + j];
#pragma unroll
            for (int j = 0; j < kKfdbNeigh; ++j) {
                ok[j] = nb[j] >= 0 && nb[j] < N;
                const orbfe_kfdb_state& ns = d.st[ok[j] ? nb[j] : s];
                ok[j] = ok[j] && (a.loop ? ns.loop_query == a.qid && ns.loop_words > min_common  // :234
                                         : ns.reloc_query == a.qid);                             // :353
                sc[j] = a.loop ? ns.loop_score : ns.reloc_score;
                set[j] = ns.scores_set & (a.loop ? 1 : 2);
            }
#pragma unroll
            for (int j = 0; j < kKfdbNeigh; ++j) {
                if (!ok[j]) continue;
                float v = sc[j];
                if (!set[j]) {  // H18: never written
                    v = 0.0f;
                    s_h18 = 1;
                }
                acc_score += v;
                if (v > best_score) {
                    bk = nb[j];
                    best_score = v;
                }
            }
            acc[e] = acc_score;
            best[e] = bk;
            if (acc_score > lmax) lmax = acc_score;
        }
        s_best[tid] = lmax;
        __syncthreads();
        for (int stride = kKfdbBlock / 2; stride > 0; stride >>= 1) {
            if (tid < stride && s_best[tid + stride] > s_best[tid]) s_best[tid] = s_best[tid + stride];
            __syncthreads();
        }
        const float retain = 0.75f * s_best[0];  // :251, :370
        for (int e = tid; e < E; e += kKfdbBlock)
            if (acc[e] > retain) atomicMin(&d.first_e[best[e]], e);
        __syncthreads();
        // the retained entries' best keyframes, each at its first occurrence (:257-268)
        int base = 0;
        for (int c = 0; c < E; c += kKfdbBlock) {
            const int e = c + tid;
            const bool keep = e < E && acc[e] > retain && d.first_e[best[e]] == e;
            int total;
            const int ex = block_exclusive_scan<kKfdbBlock>(keep ? 1 : 0, tmp, total);
            if (keep && base + ex < a.cand_cap) a.cand[base + ex] = best[e];
            base += total;
        }
        n_cand = base;
        if (s_h18) status = ORBFE_ERR_UNSUPPORTED;
    }
    __syncthreads();
    if (tid == 0) {
        *a.counter = 0;
        a.result[0] = n_cand;
        a.result[1] = status;
        __hip_atomic_store(&a.result[2], 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// KeyFrameDatabase::add (:115-121): a BowVector into slot s, validated on the way (word ids
// strictly ascending and below the vocabulary's word count); a fresh keyframe's state
// (KeyFrame.cc:35, :64: the four integers 0, the two scores not initialised).
struct KfdbSlotArgs {
    KfdbDev d;
    int slot, nwords;
    unsigned seq;
    const int* src_ids;
    const double* src_vals;
    const int* src_nw;
    int* result;  // device-mapped pinned: status, done
};

__global__ __launch_bounds__(kKfdbBlock) void kfdb_slot_kernel(KfdbSlotArgs a) {
    const KfdbDev& d = a.d;
    const int n = *a.src_nw;
    int bad = n < 0 || n > d.cap;
    if (!bad)
        for (int i = threadIdx.x; i < n; i += kKfdbBlock) {
            const int w = a.src_ids[i];
            if (w < 0 || w >= a.nwords || (i > 0 && a.src_ids[i - 1] >= w)) bad = 1;
        }
    bad = __syncthreads_or(bad);
    if (!bad)
        for (int i = threadIdx.x; i < n; i += kKfdbBlock) {
            d.ids[(size_t)a.slot * d.cap + i] = a.src_ids[i];
            d.vals[(size_t)a.slot * d.cap + i] = a.src_vals[i];
        }
    if (threadIdx.x < kKfdbNeigh) d.neigh[a.slot * kKfdbNeigh + threadIdx.x] = -1;
    __syncthreads();
    if (threadIdx.x == 0) {
        d.nw[a.slot] = bad ? 0 : n;
        d.seq[a.slot] = a.seq;
        orbfe_kfdb_state z;
        memset(&z, 0, sizeof z);
        d.st[a.slot] = z;
        a.result[0] = bad ? ORBFE_ERR_ARG : ORBFE_OK;
        __hip_atomic_store(&a.result[1], 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// KeyFrameDatabase::erase (:123-142): the slot leaves every word's list (nw = 0) and every
// covisibility list that named it.
__global__ __launch_bounds__(kKfdbBlock) void kfdb_erase_kernel(KfdbDev d, int slot) {
    const int i = blockIdx.x * kKfdbBlock + threadIdx.x;
    if (i == 0) d.nw[slot] = 0;
    if (i < d.nslots * kKfdbNeigh && d.neigh[i] == slot) d.neigh[i] = -1;
}

struct KfdbNeighList {
    int v[kKfdbNeigh];
};
__global__ void kfdb_covis_kernel(KfdbDev d, int slot, KfdbNeighList l) {
    if (threadIdx.x < kKfdbNeigh) d.neigh[slot * kKfdbNeigh + threadIdx.x] = l.v[threadIdx.x];
}

__global__ void kfdb_scores_kernel(KfdbDev d, int slot, float loop_score, float reloc_score) {
    d.st[slot].loop_score = loop_score;
    d.st[slot].reloc_score = reloc_score;
    d.st[slot].scores_set = 3;
}

}  // namespace orbfe

using namespace orbfe;

struct orbfe_kfdb {
    orbfe_vocabulary* voc = nullptr;
    int device = 0, cap = 0;
    int nalloc = 0, hi = 0, nlive = 0;
    std::vector<uint8_t> live;
    std::vector<int> free_list;  // the most recently freed slot is reused first
    uint64_t next_seq = 0;
    unsigned epoch = 0;
    DevBuf ids, vals, nw, seq, neigh, st, cnt, firstw, dscore, conn, first_e, ekey, eslot, q, counter;
    hipStream_t own = nullptr, stream = nullptr;
    uint8_t* pin = nullptr;
    uint8_t* pin_dev = nullptr;
    size_t pin_cap = 0;

    uint8_t* stage(size_t bytes) {
        if (bytes <= pin_cap) return pin;
        if (pin) {
            hipStreamSynchronize(stream);
            hipHostFree(pin);
        }
        pin = pin_dev = nullptr;
        pin_cap = 0;
        void* p = nullptr;
        void* dp = nullptr;
        const size_t n = std::max<size_t>(bytes, (size_t)128 << 10);
        if (hipHostMalloc(&p, n, hipHostMallocDefault) != hipSuccess) return nullptr;
        if (hipHostGetDevicePointer(&dp, p, 0) != hipSuccess) {
            hipHostFree(p);
            return nullptr;
        }
        pin = static_cast<uint8_t*>(p);
        pin_dev = static_cast<uint8_t*>(dp);
        pin_cap = n;
        return pin;
    }
    KfdbDev dev() const {
        return KfdbDev{cap, hi, ids.as<int>(), vals.as<double>(), nw.as<int>(), seq.as<unsigned>(),
                       neigh.as<int>(), st.as<orbfe_kfdb_state>(), cnt.as<int>(), firstw.as<int>(),
                       dscore.as<double>(), conn.as<unsigned>(), first_e.as<int>(),
                       ekey.as<unsigned long long>(), eslot.as<int>()};
    }
    bool is_live(int s) const { return s >= 0 && s < hi && live[s]; }
    ~orbfe_kfdb() {
        if (pin) hipHostFree(pin);
        if (own) hipStreamDestroy(own);
    }
};

namespace {

// Storage for n slots: the persistent arrays keep their first `hi` slots, the rest is zeroed.
int kfdb_grow(orbfe_kfdb* db, int n) {
    auto regrow = [&](DevBuf& b, size_t per_slot) -> int {
        DevBuf nb;
        int st = nb.ensure(per_slot * (size_t)n);
        if (st) return st;
        ORBFE_HIP(hipMemsetAsync(nb.p, 0, per_slot * (size_t)n, db->stream));
        if (b.p && db->hi > 0)
            ORBFE_HIP(hipMemcpyAsync(nb.p, b.p, per_slot * (size_t)db->hi, hipMemcpyDeviceToDevice,
                                     db->stream));
        ORBFE_HIP(hipStreamSynchronize(db->stream));
        b = std::move(nb);
        return ORBFE_OK;
    };
    int st;
    if ((st = regrow(db->ids, sizeof(int) * (size_t)db->cap))) return st;
    if ((st = regrow(db->vals, sizeof(double) * (size_t)db->cap))) return st;
    if ((st = regrow(db->nw, sizeof(int)))) return st;
    if ((st = regrow(db->seq, sizeof(unsigned)))) return st;
    if ((st = regrow(db->neigh, sizeof(int) * kKfdbNeigh))) return st;
    if ((st = regrow(db->st, sizeof(orbfe_kfdb_state)))) return st;
    if ((st = regrow(db->conn, sizeof(unsigned)))) return st;
    for (DevBuf* b : {&db->cnt, &db->firstw, &db->first_e})
        if ((st = b->ensure(sizeof(int) * (size_t)n))) return st;
    if ((st = db->dscore.ensure(sizeof(double) * (size_t)n))) return st;
    if ((st = db->ekey.ensure(sizeof(unsigned long long) * (size_t)std::max(n, kKfdbMaxEntries)))) return st;
    if ((st = db->eslot.ensure(sizeof(int) * (size_t)std::max(n, kKfdbMaxEntries)))) return st;
    db->nalloc = n;
    db->live.resize((size_t)n, 0);
    return ORBFE_OK;
}

// Sequence numbers are 32-bit sort-key fields: when the counter would pass them, the live slots
// are renumbered 0 .. in their order.  Not exercised by any test: it takes 2^32 adds to get here.
int kfdb_renumber(orbfe_kfdb* db) {
    std::vector<unsigned> seq((size_t)std::max(db->hi, 1));
    ORBFE_HIP(hipMemcpyAsync(seq.data(), db->seq.p, sizeof(unsigned) * (size_t)db->hi,
                             hipMemcpyDeviceToHost, db->stream));
    ORBFE_HIP(hipStreamSynchronize(db->stream));
    std::vector<int> order;
    for (int s = 0; s < db->hi; ++s)
        if (db->live[s]) order.push_back(s);
    std::sort(order.begin(), order.end(), [&](int x, int y) { return seq[x] < seq[y]; });
    for (size_t i = 0; i < order.size(); ++i) seq[order[i]] = (unsigned)i;
    ORBFE_HIP(hipMemcpyAsync(db->seq.p, seq.data(), sizeof(unsigned) * (size_t)db->hi,
                             hipMemcpyHostToDevice, db->stream));
    ORBFE_HIP(hipStreamSynchronize(db->stream));
    db->next_seq = order.size();
    return ORBFE_OK;
}

// add / add_device: the BowVector at (d_ids, d_vals, d_nw) — device memory, or the device view of
// the pinned staging block — into a free slot.
int kfdb_add(orbfe_kfdb* db, const int* d_ids, const double* d_vals, const int* d_nw, int* res,
             int* res_dev, int32_t* slot_out) {
    int st;
    if (db->next_seq >= 0xffffffffull && (st = kfdb_renumber(db))) return st;
    int slot;
    const bool reuse = !db->free_list.empty();
    if (reuse) {
        slot = db->free_list.back();
    } else {
        if (db->hi == db->nalloc && (st = kfdb_grow(db, std::max(2 * db->nalloc, 16)))) return st;
        slot = db->hi;
    }
    if (!reuse) ++db->hi;  // the kernels' slot count covers the new slot
    KfdbSlotArgs a{db->dev(), slot, db->voc->nwords, (unsigned)db->next_seq, d_ids, d_vals, d_nw, res_dev};
    res[0] = 0;
    __atomic_store_n(&res[1], -1, __ATOMIC_RELEASE);
    hipLaunchKernelGGL(kfdb_slot_kernel, dim3(1), dim3(kKfdbBlock), 0, db->stream, a);
    if (hipGetLastError() != hipSuccess) st = ORBFE_ERR_HIP;
    else st = wait_words(res + 1, 1, -1, db->stream, 2000);
    if (st == ORBFE_OK) st = res[0];
    if (st != ORBFE_OK) {
        if (!reuse) --db->hi;
        return st;
    }
    if (reuse) db->free_list.pop_back();
    db->live[slot] = 1;
    ++db->nlive;
    ++db->next_seq;
    if (slot_out) *slot_out = slot;
    return ORBFE_OK;
}

bool ascending(const int32_t* ids, int n) {
    for (int i = 1; i < n; ++i)
        if (ids[i - 1] >= ids[i]) return false;
    return true;
}

// One query.  The query vector, its count and the connected slots are device pointers; the
// candidates go to d_cand (device memory, or the device view of the pinned block).
int kfdb_query(orbfe_kfdb* db, int loop, uint64_t qid, const int* d_ids, const double* d_vals,
               const int* d_nw, int n_conn, const int* d_conn, float min_score, int* d_cand,
               int cand_cap, int* res, int* res_dev, int32_t* n_cand) {
    orbfe_vocabulary* v = db->voc;
    *n_cand = 0;
    if (v->scoring == 3) return ORBFE_ERR_UNSUPPORTED;
    int st;
    if (!db->nalloc && (st = kfdb_grow(db, 16))) return st;
    if (++db->epoch == 0) {  // the stamps of 2^32 calls ago
        ORBFE_HIP(hipMemsetAsync(db->conn.p, 0, sizeof(unsigned) * (size_t)db->nalloc, db->stream));
        db->epoch = 1;
    }
    KfdbQuery a;
    a.d = db->dev();
    a.loop = loop;
    a.qid = qid;
    a.q_ids = d_ids;
    a.q_vals = d_vals;
    a.q_nw = d_nw;
    a.n_conn = n_conn;
    a.conn_slots = d_conn;
    a.epoch = db->epoch;
    a.min_score = min_score;
    a.scoring = v->scoring;
    a.fused = v->arith == ORBFE_ARITH_X86_SIMD && (v->scoring == 1 || v->scoring == 5);
    a.cand = d_cand;
    a.cand_cap = cand_cap;
    a.result = res_dev;
    a.counter = db->counter.as<int>();
    res[0] = res[1] = 0;
    __atomic_store_n(&res[2], -1, __ATOMIC_RELEASE);
    const int per = kKfdbBlock / 64;
    hipLaunchKernelGGL(kfdb_score_kernel, dim3(std::max(1, (db->hi + per - 1) / per)),
                       dim3(kKfdbBlock), 0, db->stream, a);
    if (hipGetLastError() != hipSuccess) return ORBFE_ERR_HIP;
    if ((st = wait_words(res + 2, 1, -1, db->stream, 5000))) return st;
    *n_cand = res[0];
    if (res[1] == ORBFE_ERR_CAPACITY || res[0] > cand_cap) return ORBFE_ERR_CAPACITY;
    return res[1];
}

// The host forms' pinned block: result words | candidates | query count, values, ids, connected.
constexpr size_t kKfdbResBytes = 64;
constexpr size_t kKfdbCandOff = kKfdbResBytes;
constexpr size_t kKfdbUpOff = kKfdbCandOff + sizeof(int) * kKfdbMaxEntries;

int kfdb_query_host(orbfe_kfdb* db, int loop, uint64_t qid, const int32_t* ids,
                    const double* vals, int nw, int n_conn, const int32_t* conn, float min_score,
                    int32_t* cand, int cand_cap, int32_t* n_cand) {
    if (!db || !n_cand || nw < 0 || nw > db->cap || (nw && (!ids || !vals)) || n_conn < 0 ||
        (n_conn && !conn) || cand_cap < 0 || (cand_cap && !cand) || !ascending(ids, nw))
        return ORBFE_ERR_ARG;
    DeviceGuard dg(db->device);
    const size_t o_vals = 8, o_ids = o_vals + sizeof(double) * (size_t)nw,
                 o_conn = o_ids + sizeof(int) * (size_t)nw,
                 up = (o_conn + sizeof(int) * (size_t)n_conn + 7) & ~(size_t)7;
    uint8_t* p = db->stage(kKfdbUpOff + up);
    if (!p) return ORBFE_ERR_NOMEM;
    int st;
    if ((st = db->q.ensure(std::max<size_t>(up, 4096)))) return st;
    uint8_t* u = p + kKfdbUpOff;
    *reinterpret_cast<int*>(u) = nw;
    if (nw) {
        std::memcpy(u + o_vals, vals, sizeof(double) * (size_t)nw);
        std::memcpy(u + o_ids, ids, sizeof(int) * (size_t)nw);
    }
    if (n_conn) std::memcpy(u + o_conn, conn, sizeof(int) * (size_t)n_conn);
    ORBFE_HIP(hipMemcpyAsync(db->q.p, u, up, hipMemcpyHostToDevice, db->stream));
    const uint8_t* dq = db->q.as<uint8_t>();
    st = kfdb_query(db, loop, qid, reinterpret_cast<const int*>(dq + o_ids),
                    reinterpret_cast<const double*>(dq + o_vals), reinterpret_cast<const int*>(dq),
                    n_conn, reinterpret_cast<const int*>(dq + o_conn), min_score,
                    reinterpret_cast<int*>(db->pin_dev + kKfdbCandOff), kKfdbMaxEntries,
                    reinterpret_cast<int*>(p), reinterpret_cast<int*>(db->pin_dev), n_cand);
    if (st != ORBFE_OK && st != ORBFE_ERR_UNSUPPORTED) return st;
    if (*n_cand > cand_cap) return ORBFE_ERR_CAPACITY;
    if (*n_cand) std::memcpy(cand, p + kKfdbCandOff, sizeof(int) * (size_t)*n_cand);
    return st;
}

int kfdb_query_device(orbfe_kfdb* db, int loop, uint64_t qid, const int32_t* d_ids,
                      const double* d_vals, const int32_t* d_nw, int n_conn,
                      const int32_t* d_conn, float min_score, int32_t* d_cand, int cand_cap,
                      int32_t* n_cand) {
    if (!db || !n_cand || !d_ids || !d_vals || !d_nw || n_conn < 0 || (n_conn && !d_conn) ||
        cand_cap < 0 || (cand_cap && !d_cand))
        return ORBFE_ERR_ARG;
    DeviceGuard dg(db->device);
    uint8_t* p = db->stage(kKfdbResBytes);
    if (!p) return ORBFE_ERR_NOMEM;
    return kfdb_query(db, loop, qid, d_ids, d_vals, d_nw, n_conn, d_conn, min_score, d_cand,
                      cand_cap, reinterpret_cast<int*>(p), reinterpret_cast<int*>(db->pin_dev),
                      n_cand);
}

}  // namespace

extern "C" {

int orbfe_vocabulary_set_arithmetic(orbfe_vocabulary* v, int mode) {
    if (!v || (mode != ORBFE_ARITH_SCALAR && mode != ORBFE_ARITH_X86_SIMD)) return ORBFE_ERR_ARG;
    v->arith = mode;
    return ORBFE_OK;
}

int orbfe_vocabulary_score_batch_device(orbfe_vocabulary* v, int n_pairs, const int32_t* d_pair_a,
                                        const int32_t* d_pair_b, int cap,
                                        const int32_t* d_word_ids, const double* d_values,
                                        const int32_t* d_nw, double* d_score) {
    if (!v || n_pairs < 0 || cap < 1 || (n_pairs && (!d_pair_a || !d_pair_b || !d_word_ids ||
                                                     !d_values || !d_nw || !d_score)))
        return ORBFE_ERR_ARG;
    if (v->scoring == 3) return ORBFE_ERR_UNSUPPORTED;
    if (!n_pairs) return ORBFE_OK;
    DeviceGuard dg(v->device);
    ScorePairsArgs a{n_pairs, cap, v->scoring,
                     v->arith == ORBFE_ARITH_X86_SIMD && (v->scoring == 1 || v->scoring == 5),
                     d_pair_a, d_pair_b, d_word_ids, d_values, d_nw, d_score};
    const int per = kKfdbBlock / 64;
    hipLaunchKernelGGL(bow_score_pairs_kernel, dim3((n_pairs + per - 1) / per), dim3(kKfdbBlock), 0,
                       v->stream, a);
    ORBFE_HIP(hipGetLastError());
    return ORBFE_OK;
}

int orbfe_vocabulary_score(orbfe_vocabulary* v, const int32_t* ids1, const double* vals1, int n1,
                           const int32_t* ids2, const double* vals2, int n2, double* score) {
    if (!v || !score || n1 < 0 || n2 < 0 || (n1 && (!ids1 || !vals1)) || (n2 && (!ids2 || !vals2)) ||
        !ascending(ids1, n1) || !ascending(ids2, n2))
        return ORBFE_ERR_ARG;
    if (v->scoring == 3) return ORBFE_ERR_UNSUPPORTED;
    DeviceGuard dg(v->device);
    // two slots of capacity cap: values | ids | counts | pair | score
    const int cap = std::max(std::max(n1, n2), 1);
    const size_t o_ids = sizeof(double) * 2 * (size_t)cap, o_nw = o_ids + sizeof(int) * 2 * (size_t)cap,
                 o_pair = o_nw + 8, o_score = o_pair + 8, bytes = o_score + 8;
    std::vector<uint8_t> h(bytes, 0);
    if (n1) {
        std::memcpy(h.data(), vals1, sizeof(double) * (size_t)n1);
        std::memcpy(h.data() + o_ids, ids1, sizeof(int) * (size_t)n1);
    }
    if (n2) {
        std::memcpy(h.data() + sizeof(double) * (size_t)cap, vals2, sizeof(double) * (size_t)n2);
        std::memcpy(h.data() + o_ids + sizeof(int) * (size_t)cap, ids2, sizeof(int) * (size_t)n2);
    }
    int* hn = reinterpret_cast<int*>(h.data() + o_nw);
    hn[0] = n1;
    hn[1] = n2;
    reinterpret_cast<int*>(h.data() + o_pair)[1] = 1;
    int st;
    if ((st = v->k_score.ensure(bytes))) return st;
    uint8_t* dp = v->k_score.as<uint8_t>();
    ORBFE_HIP(hipMemcpyAsync(dp, h.data(), bytes, hipMemcpyHostToDevice, v->stream));
    st = orbfe_vocabulary_score_batch_device(
        v, 1, reinterpret_cast<int*>(dp + o_pair), reinterpret_cast<int*>(dp + o_pair) + 1, cap,
        reinterpret_cast<int*>(dp + o_ids), reinterpret_cast<double*>(dp),
        reinterpret_cast<int*>(dp + o_nw), reinterpret_cast<double*>(dp + o_score));
    if (st) return st;
    ORBFE_HIP(hipMemcpyAsync(score, dp + o_score, sizeof(double), hipMemcpyDeviceToHost, v->stream));
    ORBFE_HIP(hipStreamSynchronize(v->stream));
    return ORBFE_OK;
}

orbfe_kfdb* orbfe_kfdb_create(orbfe_vocabulary* voc, int cap, int slots_hint, int* status) {
    int st = ORBFE_OK;
    orbfe_kfdb* db = nullptr;
    try {
        if (!voc || cap < 1 || cap > kKfdbMaxWords || slots_hint < 0) st = ORBFE_ERR_ARG;
        if (st == ORBFE_OK) {
            DeviceGuard dg(voc->device);
            db = new orbfe_kfdb();
            db->voc = voc;
            db->device = voc->device;
            db->cap = cap;
            if (hipStreamCreateWithFlags(&db->own, hipStreamNonBlocking) != hipSuccess) st = ORBFE_ERR_HIP;
            db->stream = db->own;
            if (st == ORBFE_OK) st = db->counter.ensure(64);
            if (st == ORBFE_OK && hipMemsetAsync(db->counter.p, 0, 64, db->stream) != hipSuccess)
                st = ORBFE_ERR_HIP;
            if (st == ORBFE_OK && !db->stage(kKfdbUpOff + 64 * 1024)) st = ORBFE_ERR_NOMEM;
            if (st == ORBFE_OK) st = kfdb_grow(db, std::max(slots_hint, 16));
        }
    } catch (const std::bad_alloc&) {
        st = ORBFE_ERR_NOMEM;
    } catch (...) {
        st = ORBFE_ERR_HIP;
    }
    if (st != ORBFE_OK && db) {
        delete db;
        db = nullptr;
    }
    if (status) *status = st;
    return db;
}

void orbfe_kfdb_destroy(orbfe_kfdb* db) {
    if (!db) return;
    DeviceGuard dg(db->device);
    if (db->stream) hipStreamSynchronize(db->stream);
    delete db;
}

int orbfe_kfdb_set_stream(orbfe_kfdb* db, void* hip_stream) {
    if (!db) return ORBFE_ERR_ARG;
    DeviceGuard dg(db->device);
    hipStreamSynchronize(db->stream);
    db->stream = hip_stream ? static_cast<hipStream_t>(hip_stream) : db->own;
    return ORBFE_OK;
}

int orbfe_kfdb_size(const orbfe_kfdb* db) { return db ? db->nlive : ORBFE_ERR_ARG; }

int orbfe_kfdb_add(orbfe_kfdb* db, const int32_t* word_ids, const double* values, int nw,
                   int32_t* slot) {
    if (!db || !slot || nw < 0 || nw > db->cap || (nw && (!word_ids || !values)) ||
        !ascending(word_ids, nw) || (nw && (word_ids[0] < 0 || word_ids[nw - 1] >= db->voc->nwords)))
        return ORBFE_ERR_ARG;
    try {
        DeviceGuard dg(db->device);
        const size_t o_vals = 64, o_ids = o_vals + sizeof(double) * (size_t)nw;
        uint8_t* p = db->stage(kKfdbUpOff + o_ids + sizeof(int) * (size_t)nw);
        if (!p) return ORBFE_ERR_NOMEM;
        uint8_t* u = p + kKfdbUpOff;
        *reinterpret_cast<int*>(u) = nw;
        if (nw) {
            std::memcpy(u + o_vals, values, sizeof(double) * (size_t)nw);
            std::memcpy(u + o_ids, word_ids, sizeof(int) * (size_t)nw);
        }
        const uint8_t* du = db->pin_dev + kKfdbUpOff;
        return kfdb_add(db, reinterpret_cast<const int*>(du + o_ids),
                        reinterpret_cast<const double*>(du + o_vals), reinterpret_cast<const int*>(du),
                        reinterpret_cast<int*>(p), reinterpret_cast<int*>(db->pin_dev), slot);
    } catch (const std::bad_alloc&) {
        return ORBFE_ERR_NOMEM;
    }
}

int orbfe_kfdb_add_device(orbfe_kfdb* db, const int32_t* d_word_ids, const double* d_values,
                          const int32_t* d_nw, int32_t* slot) {
    if (!db || !slot || !d_word_ids || !d_values || !d_nw) return ORBFE_ERR_ARG;
    try {
        DeviceGuard dg(db->device);
        uint8_t* p = db->stage(kKfdbResBytes);
        if (!p) return ORBFE_ERR_NOMEM;
        return kfdb_add(db, d_word_ids, d_values, d_nw, reinterpret_cast<int*>(p),
                        reinterpret_cast<int*>(db->pin_dev), slot);
    } catch (const std::bad_alloc&) {
        return ORBFE_ERR_NOMEM;
    }
}

int orbfe_kfdb_erase(orbfe_kfdb* db, int slot) {
    if (!db || !db->is_live(slot)) return ORBFE_ERR_ARG;
    DeviceGuard dg(db->device);
    hipLaunchKernelGGL(kfdb_erase_kernel, dim3((db->hi * kKfdbNeigh + kKfdbBlock - 1) / kKfdbBlock),
                       dim3(kKfdbBlock), 0, db->stream, db->dev(), slot);
    ORBFE_HIP(hipGetLastError());
    db->live[slot] = 0;
    --db->nlive;
    db->free_list.push_back(slot);
    return ORBFE_OK;
}

int orbfe_kfdb_clear(orbfe_kfdb* db) {
    if (!db) return ORBFE_ERR_ARG;
    DeviceGuard dg(db->device);
    if (db->hi) ORBFE_HIP(hipMemsetAsync(db->nw.p, 0, sizeof(int) * (size_t)db->hi, db->stream));
    std::fill(db->live.begin(), db->live.end(), 0);
    db->free_list.clear();
    db->hi = 0;
    db->nlive = 0;
    return ORBFE_OK;
}

int orbfe_kfdb_set_covisibility(orbfe_kfdb* db, int slot, int n, const int32_t* neigh_slots) {
    if (!db || !db->is_live(slot) || n < 0 || n > kKfdbNeigh || (n && !neigh_slots))
        return ORBFE_ERR_ARG;
    KfdbNeighList l;
    for (int j = 0; j < kKfdbNeigh; ++j) {
        l.v[j] = j < n ? neigh_slots[j] : -1;
        if (l.v[j] != -1 && !db->is_live(l.v[j])) return ORBFE_ERR_ARG;
    }
    DeviceGuard dg(db->device);
    hipLaunchKernelGGL(kfdb_covis_kernel, dim3(1), dim3(64), 0, db->stream, db->dev(), slot, l);
    ORBFE_HIP(hipGetLastError());
    return ORBFE_OK;
}

int orbfe_kfdb_set_scores(orbfe_kfdb* db, int slot, float loop_score, float reloc_score) {
    if (!db || !db->is_live(slot)) return ORBFE_ERR_ARG;
    DeviceGuard dg(db->device);
    hipLaunchKernelGGL(kfdb_scores_kernel, dim3(1), dim3(1), 0, db->stream, db->dev(), slot,
                       loop_score, reloc_score);
    ORBFE_HIP(hipGetLastError());
    return ORBFE_OK;
}

int orbfe_kfdb_get_state(orbfe_kfdb* db, int slot, orbfe_kfdb_state* state) {
    if (!db || !state || !db->is_live(slot)) return ORBFE_ERR_ARG;
    DeviceGuard dg(db->device);
    ORBFE_HIP(hipMemcpyAsync(state, db->st.as<orbfe_kfdb_state>() + slot, sizeof *state,
                             hipMemcpyDeviceToHost, db->stream));
    ORBFE_HIP(hipStreamSynchronize(db->stream));
    return ORBFE_OK;
}

int orbfe_kfdb_detect_loop_candidates(orbfe_kfdb* db, uint64_t query_id, const int32_t* word_ids,
                                      const double* values, int nw, int n_conn,
                                      const int32_t* conn_slots, float min_score, int32_t* cand,
                                      int cand_cap, int32_t* n_cand) {
    return kfdb_query_host(db, 1, query_id, word_ids, values, nw, n_conn, conn_slots, min_score,
                           cand, cand_cap, n_cand);
}

int orbfe_kfdb_detect_relocalization_candidates(orbfe_kfdb* db, uint64_t frame_id,
                                                const int32_t* word_ids, const double* values,
                                                int nw, int32_t* cand, int cand_cap,
                                                int32_t* n_cand) {
    return kfdb_query_host(db, 0, frame_id, word_ids, values, nw, 0, nullptr, 0.f, cand, cand_cap,
                           n_cand);
}

int orbfe_kfdb_detect_loop_candidates_device(orbfe_kfdb* db, uint64_t query_id,
                                             const int32_t* d_word_ids, const double* d_values,
                                             const int32_t* d_nw, int n_conn,
                                             const int32_t* d_conn_slots, float min_score,
                                             int32_t* d_cand, int cand_cap, int32_t* n_cand) {
    return kfdb_query_device(db, 1, query_id, d_word_ids, d_values, d_nw, n_conn, d_conn_slots,
                             min_score, d_cand, cand_cap, n_cand);
}

int orbfe_kfdb_detect_relocalization_candidates_device(orbfe_kfdb* db, uint64_t frame_id,
                                                       const int32_t* d_word_ids,
                                                       const double* d_values,
                                                       const int32_t* d_nw, int32_t* d_cand,
                                                       int cand_cap, int32_t* n_cand) {
    return kfdb_query_device(db, 0, frame_id, d_word_ids, d_values, d_nw, 0, nullptr, 0.f, d_cand,
                             cand_cap, n_cand);
}

}  // extern "C"
