// The C++ adapter's ORBVocabulary::score and KeyFrameDatabase (include/orbfe_orbslam.hpp) on a
// script dumped by tests/test_gpu_kfdb_cpp.py, checked here against a plain std::list inverted
// file: a restatement of KeyFrameDatabase.cc:115-389 and ScoringObject.cpp:23-311 (the lines are
// cited where they are followed), with the state fields of KeyFrame.h:166-171 per keyframe.
//
//   kfdb_test <vocabulary.txt> <script.bin>   runs every operation on both and compares each
//                                             query's candidate ids, their order and the
//                                             uninitialised-score flag; prints "KFDB DONE".
//   kfdb_test --time <script.bin> [reps]      times the inverted-file walk alone (one thread, no
//                                             device): ms per pass over the script's queries.
//
// Script (little-endian): int32 scoring, n_ops; per operation int32 kind, then
//   0 add    int64 id, int32 nw, int32 ids[nw], double values[nw]
//   1 erase  int64 id
//   2 covis  int64 id, int32 n, int64 ids[n]          (an id not in the database: skipped)
//   3 reloc  int64 id, int32 nw, ids, values
//   4 loop   int64 id, int32 nw, ids, values, int32 n_conn, int64 conn[n_conn], float min_score
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <list>
#include <map>
#include <set>
#include <string>
#include <vector>

#include "../../include/orbfe_orbslam.hpp"

namespace {

struct Op {
    int kind = 0;
    int64_t id = 0;
    orbfe::BowVector bow;
    std::vector<int64_t> ids;  // covisibility list / connected keyframes
    float min_score = 0.f;
};

template <class T>
std::vector<T> rd(FILE* f, size_t n) {
    std::vector<T> v(n);
    if (n && std::fread(v.data(), sizeof(T), n, f) != n) {
        std::fprintf(stderr, "kfdb_test: short script\n");
        std::exit(2);
    }
    return v;
}

std::vector<Op> read_script(const char* path, int& scoring) {
    FILE* f = std::fopen(path, "rb");
    if (!f) {
        std::fprintf(stderr, "kfdb_test: cannot open %s\n", path);
        std::exit(2);
    }
    const std::vector<int32_t> h = rd<int32_t>(f, 2);
    scoring = h[0];
    std::vector<Op> ops((size_t)h[1]);
    for (Op& o : ops) {
        o.kind = rd<int32_t>(f, 1)[0];
        o.id = rd<int64_t>(f, 1)[0];
        if (o.kind == 0 || o.kind == 3 || o.kind == 4) {
            const int nw = rd<int32_t>(f, 1)[0];
            o.bow.ids = rd<int32_t>(f, (size_t)nw);
            o.bow.values = rd<double>(f, (size_t)nw);
        }
        if (o.kind == 2 || o.kind == 4) {
            const int n = rd<int32_t>(f, 1)[0];
            o.ids = rd<int64_t>(f, (size_t)n);
        }
        if (o.kind == 4) o.min_score = rd<float>(f, 1)[0];
    }
    std::fclose(f);
    return ops;
}

// ScoringObject.cpp:23-311: the merge walk visits the common words in ascending order; one double
// accumulator; the L2 and dot-product products are contracted into the add (fma), as the
// reference's -O3 -march=native build compiles :91 and :290.
double score_restated(int scoring, const orbfe::BowVector& a, const orbfe::BowVector& b) {
    double s = 0.0;
    size_t i = 0, j = 0;
    while (i < a.ids.size() && j < b.ids.size()) {
        if (a.ids[i] < b.ids[j]) { ++i; continue; }
        if (a.ids[i] > b.ids[j]) { ++j; continue; }
        const double vi = a.values[i], wi = b.values[j];
        switch (scoring) {
            case 0: s += std::fabs(vi - wi) - std::fabs(vi) - std::fabs(wi); break;  // :41
            case 2: if (vi + wi != 0.0) s += vi * wi / (vi + wi); break;            // :148
            case 4: s += std::sqrt(vi * wi); break;                                  // :245
            default: s = std::fma(vi, wi, s); break;                                 // :91, :290
        }
        ++i;
        ++j;
    }
    if (scoring == 0) s = -s / 2.0;                                                  // :65
    if (scoring == 1) s = s >= 1 ? 1.0 : 1.0 - std::sqrt(1.0 - s);                   // :114-117
    if (scoring == 2) s = 2. * s;                                                    // :167
    return s;
}

struct KF {
    int64_t id;
    orbfe::BowVector bow;
    uint64_t loop_query = 0, reloc_query = 0;  // KeyFrame.cc:35, :64
    int loop_words = 0, reloc_words = 0;
    float loop_score = 0.f, reloc_score = 0.f;  // not initialised by the reference: flags below
    bool loop_set = false, reloc_set = false;
    std::vector<int64_t> neigh;
};

struct ListDb {
    int scoring;
    std::map<int32_t, std::list<KF*>> inv;  // mvInvertedFile
    std::map<int64_t, KF*> kfs;
    explicit ListDb(int sc) : scoring(sc) {}
    ~ListDb() {
        for (auto& p : kfs) delete p.second;
    }
    void add(int64_t id, const orbfe::BowVector& bow) {  // :115-121
        KF* k = new KF{id, bow};
        kfs[id] = k;
        for (int32_t w : bow.ids) inv[w].push_back(k);
    }
    void erase(int64_t id) {  // :123-142
        KF* k = kfs.at(id);
        for (int32_t w : k->bow.ids) inv[w].remove(k);
        kfs.erase(id);
        delete k;
    }
    KF* find(int64_t id) const {
        auto it = kfs.find(id);
        return it == kfs.end() ? nullptr : it->second;
    }

    // :219-271 / :338-388
    std::vector<int64_t> tail(bool loop, uint64_t qid, const std::list<std::pair<float, KF*>>& scored,
                              int min_common, float best_acc, bool& h18) const {
        std::list<std::pair<float, KF*>> acc_list;
        for (const auto& e : scored) {
            KF* k = e.second;
            float best_score = e.first, acc = e.first;
            KF* best = k;
            for (size_t j = 0; j < k->neigh.size() && j < 10; ++j) {
                KF* n = find(k->neigh[j]);
                if (!n) continue;
                if (loop ? !(n->loop_query == qid && n->loop_words > min_common)  // :234
                         : n->reloc_query != qid)                                 // :353
                    continue;
                float v = loop ? n->loop_score : n->reloc_score;
                if (!(loop ? n->loop_set : n->reloc_set)) {
                    v = 0.f;
                    h18 = true;
                }
                acc += v;
                if (v > best_score) {
                    best = n;
                    best_score = v;
                }
            }
            acc_list.push_back({acc, best});
            if (acc > best_acc) best_acc = acc;
        }
        const float retain = 0.75f * best_acc;  // :251 / :370
        std::set<KF*> seen;
        std::vector<int64_t> out;
        for (const auto& e : acc_list)
            if (e.first > retain && seen.insert(e.second).second) out.push_back(e.second->id);
        return out;
    }

    std::vector<int64_t> detect_loop(uint64_t qid, const orbfe::BowVector& q,
                                     const std::vector<int64_t>& connected, float min_score,
                                     bool& h18) {
        std::set<KF*> conn;
        for (int64_t c : connected)
            if (find(c)) conn.insert(find(c));
        std::list<KF*> sharing;
        for (int32_t w : q.ids) {  // :161-179
            auto it = inv.find(w);
            if (it == inv.end()) continue;
            for (KF* k : it->second) {
                if (k->loop_query != qid) {
                    k->loop_words = 0;
                    if (!conn.count(k)) {
                        k->loop_query = qid;
                        sharing.push_back(k);
                    }
                }
                k->loop_words++;
            }
        }
        if (sharing.empty()) return {};  // :182
        int max_common = 0;
        for (KF* k : sharing) max_common = std::max(max_common, k->loop_words);
        const int min_common = max_common * 0.8f;  // :195
        std::list<std::pair<float, KF*>> scored;
        for (KF* k : sharing)
            if (k->loop_words > min_common) {  // :204
                const float si = (float)score_restated(scoring, q, k->bow);
                k->loop_score = si;
                k->loop_set = true;
                if (si >= min_score) scored.push_back({si, k});  // :211
            }
        if (scored.empty()) return {};  // :216
        return tail(true, qid, scored, min_common, min_score, h18);
    }

    std::vector<int64_t> detect_reloc(uint64_t qid, const orbfe::BowVector& q, bool& h18) {
        std::list<KF*> sharing;
        for (int32_t w : q.ids) {  // :282-302
            auto it = inv.find(w);
            if (it == inv.end()) continue;
            for (KF* k : it->second) {
                if (k->reloc_query != qid) {
                    k->reloc_words = 0;
                    k->reloc_query = qid;
                    sharing.push_back(k);
                }
                k->reloc_words++;
            }
        }
        if (sharing.empty()) return {};  // :304
        int max_common = 0;
        for (KF* k : sharing) max_common = std::max(max_common, k->reloc_words);
        const int min_common = max_common * 0.8f;  // :315
        std::list<std::pair<float, KF*>> scored;
        for (KF* k : sharing)
            if (k->reloc_words > min_common) {  // :326
                const float si = (float)score_restated(scoring, q, k->bow);
                k->reloc_score = si;
                k->reloc_set = true;
                scored.push_back({si, k});
            }
        if (scored.empty()) return {};  // :335
        return tail(false, qid, scored, min_common, 0.f, h18);
    }
};

int time_mode(const char* path, int reps) {
    int scoring = 0;
    const std::vector<Op> ops = read_script(path, scoring);
    ListDb ref(scoring);
    size_t nq = 0, ncand = 0;
    for (const Op& o : ops) {
        if (o.kind == 0) ref.add(o.id, o.bow);
        if (o.kind == 2 && ref.find(o.id)) ref.find(o.id)->neigh = o.ids;
    }
    const auto t0 = std::chrono::steady_clock::now();
    for (int r = 0; r < reps; ++r)
        for (const Op& o : ops) {
            bool h18 = false;
            // a fresh id per repetition, as successive frames have
            const uint64_t qid = (uint64_t)o.id + 1000u * (uint64_t)(r + 1);
            if (o.kind == 3) ncand += ref.detect_reloc(qid, o.bow, h18).size(), ++nq;
            if (o.kind == 4) ncand += ref.detect_loop(qid, o.bow, o.ids, o.min_score, h18).size(), ++nq;
        }
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    std::printf("TIME keyframes=%zu queries=%zu candidates=%zu ms_per_pass=%.6f\n", ref.kfs.size(),
                nq, ncand, ms / reps);
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc >= 3 && std::strcmp(argv[1], "--time") == 0)
        return time_mode(argv[2], argc > 3 ? std::atoi(argv[3]) : 10);
    if (argc < 3) return 2;
    int scoring = 0;
    const std::vector<Op> ops = read_script(argv[2], scoring);
    try {
        orbfe::ORBVocabulary voc(argv[1]);
        orbfe::KeyFrameDatabase db(voc, 4096);
        ListDb ref(scoring);
        int nq = 0, nonempty = 0, nscore = 0, bad = 0;
        const orbfe::BowVector* prev = nullptr;
        for (const Op& o : ops) {
            if (o.kind == 0) {
                db.add((uint64_t)o.id, o.bow);
                ref.add(o.id, o.bow);
                if (prev) {  // ORBVocabulary::score, bit for bit
                    const double g = voc.score(*prev, o.bow), w = score_restated(scoring, *prev, o.bow);
                    if (std::memcmp(&g, &w, sizeof g) != 0) {
                        std::printf("SCORE MISMATCH %.17g %.17g\n", g, w);
                        ++bad;
                    }
                    ++nscore;
                }
                prev = &o.bow;
                bool refused = false;
                try {
                    db.add((uint64_t)o.id, o.bow);  // an id already present
                } catch (const orbfe::Error& e) {
                    refused = e.status == ORBFE_ERR_UNSUPPORTED;
                }
                if (!refused) {
                    std::printf("DUPLICATE ADD ACCEPTED\n");
                    ++bad;
                }
            } else if (o.kind == 1) {
                db.erase((uint64_t)o.id);
                // the library scrubs an erased keyframe from the covisibility lists; here the
                // lists hold ids and find() skips the ones that are gone
                ref.erase(o.id);
            } else if (o.kind == 2) {
                db.SetBestCovisibilityKeyFrames((uint64_t)o.id, std::vector<uint64_t>(o.ids.begin(), o.ids.end()));
                ref.find(o.id)->neigh = o.ids;
            } else {
                bool gh = false, wh = false;
                std::vector<uint64_t> got;
                std::vector<int64_t> want;
                if (o.kind == 3) {
                    got = db.DetectRelocalizationCandidates((uint64_t)o.id, o.bow, &gh);
                    want = ref.detect_reloc((uint64_t)o.id, o.bow, wh);
                } else {
                    got = db.DetectLoopCandidates((uint64_t)o.id, o.bow,
                                                  std::vector<uint64_t>(o.ids.begin(), o.ids.end()),
                                                  o.min_score, &gh);
                    want = ref.detect_loop((uint64_t)o.id, o.bow, o.ids, o.min_score, wh);
                }
                bool same = gh == wh && got.size() == want.size();
                for (size_t i = 0; same && i < got.size(); ++i) same = got[i] == (uint64_t)want[i];
                std::printf("Q %d kind=%d n=%zu h18=%d %s\n", nq, o.kind, want.size(), (int)wh,
                            same ? "ok" : "MISMATCH");
                bad += !same;
                ++nq;
                nonempty += !want.empty();
            }
        }
        std::printf("KFDB DONE queries=%d nonempty=%d scores=%d bad=%d\n", nq, nonempty, nscore, bad);
        return bad ? 1 : 0;
    } catch (const orbfe::Error& e) {
        std::printf("ERROR %s\n", e.what());
        return 3;
    }
}
