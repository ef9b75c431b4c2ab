// map_store_plan_test — the arithmetic under the device map's store (csrc/orbfe_map_plan.hpp) on
// the CPU: the row-table planner in both of its parameterisations, the side pools' sizes and the
// column groups' growth.  No device, no library: built alone (tests/test_map_store_plan.py does
// it with -fsanitize=address,undefined) and run as a program.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>
#include <utility>
#include <vector>

#include "../../orbslam_mapsave_amd/csrc/orbfe_map_plan.hpp"

using namespace orbfe;

static int g_failed = 0;
#define CHECK(c)                                                       \
    do {                                                               \
        if (!(c)) {                                                    \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            if (++g_failed > 20) std::exit(1);                         \
        }                                                              \
    } while (0)

static bool pow2(long long v) { return v > 0 && (v & (v - 1)) == 0; }

// What holds after every batch, whatever the batch was.
static void check_table(const RowTable& t, const RowTable& before, const RowPlan& plan, long long old_alloc) {
    const size_t rows = t.off.size();
    CHECK(t.cap.size() == rows && t.len.size() == rows);
    CHECK(t.used <= t.alloc);
    std::vector<std::pair<long long, long long>> regions;
    long long live = 0;
    for (size_t r = 0; r < rows; ++r) {
        CHECK(t.len[r] >= 0 && t.len[r] <= t.cap[r]);
        if (!t.cap[r]) continue;
        CHECK(pow2(t.cap[r]) && t.cap[r] >= t.min_cap);
        const long long size = (long long)t.lanes * t.cap[r];
        CHECK(t.off[r] >= 0 && t.off[r] + size <= t.used);
        regions.push_back({t.off[r], t.off[r] + size});
        live += size;
    }
    std::sort(regions.begin(), regions.end());
    for (size_t i = 1; i < regions.size(); ++i) CHECK(regions[i - 1].second <= regions[i].first);
    CHECK(t.used <= 2 * live + t.first_alloc);
    // a row that did not outgrow its region kept it; a row that did is in the plan, once
    std::set<int> moved;
    for (const RowMove& v : plan.moves) {
        CHECK(moved.insert(v.row).second);
        CHECK(t.off[v.row] == v.new_off && t.cap[v.row] == v.new_cap);
        CHECK(v.new_off >= before.used);  // at the pool's end: an old region is not reused
    }
    for (size_t r = 0; r < before.off.size(); ++r)
        if (!moved.count((int)r)) CHECK(t.off[r] == before.off[r] && t.cap[r] == before.cap[r]);
    // the pool grows to the smallest doubling from the old size (or the first size) that holds `used`
    CHECK(plan.used == t.used && plan.alloc == t.alloc);
    if (t.used <= old_alloc) CHECK(t.alloc == old_alloc);
    else {
        long long want = old_alloc ? 2 * old_alloc : t.first_alloc;
        if (want < t.first_alloc) want = t.first_alloc;
        while (want < t.used) want *= 2;
        CHECK(t.alloc == want);
    }
    // a side pool holds what its table holds, and keeps no more than it has
    const SidePoolPlan s = side_pool_plan(t, old_alloc);
    CHECK(s.alloc == t.alloc);
    CHECK(s.keep == std::min(t.used, old_alloc));
}

// Seeded random batches of row changes over distinct rows: whole-row writes that grow or shrink,
// partial writes that leave the length, rows beyond the current count, capacity-only requests.
static void random_run(int lanes, int min_cap, long long first_alloc, unsigned seed, int batches) {
    std::mt19937 rng(seed);
    RowTable t(lanes, min_cap, first_alloc);
    for (int b = 0; b < batches; ++b) {
        const RowTable before = t;
        const int rows_now = (int)t.off.size();
        std::set<int> rows;
        const int n = std::min(1 + (int)(rng() % 12), rows_now + 6);
        while ((int)rows.size() < n) rows.insert((int)(rng() % (unsigned)(rows_now + 6)));
        std::vector<RowNeed> need;
        for (int r : rows) {
            const int old_len = before.length(r);
            const int old_cap = (size_t)r < before.cap.size() ? before.cap[r] : 0;
            int len;
            switch (rng() % 5) {
                case 0: len = -1; break;                                         // partial: length unchanged
                case 1: len = old_len ? (int)(rng() % (unsigned)old_len) : 0; break;  // shrink
                case 2: len = old_cap + 1 + (int)(rng() % 40); break;            // outgrows its region
                case 3: len = rng() % 64 == 0 ? 3000 + (int)(rng() % 3000) : (int)(rng() % 70); break;
                default: len = (int)(rng() % (unsigned)(old_cap + 1)); break;    // fits
            }
            // the graph's form: entries wanted, the length not the table's business
            if (lanes == 4) need.push_back({r, len < 0 ? 0 : len, -1});
            else need.push_back({r, 0, len});
        }
        const long long old_alloc = t.alloc;
        const RowPlan plan = t.plan(need);
        CHECK(t.used == before.used && t.alloc == old_alloc);  // until commit: the growth copies the old extent
        t.commit(plan);
        check_table(t, before, plan, old_alloc);
        for (const RowNeed& x : need) {
            const int want_len = x.new_len >= 0 ? x.new_len : before.length(x.row);
            CHECK(t.len[x.row] == want_len);
            CHECK(t.cap[x.row] >= std::max(want_len, x.entries));
            const int old_cap = (size_t)x.row < before.cap.size() ? before.cap[x.row] : 0;
            if (std::max(want_len, x.entries) <= old_cap)
                CHECK(t.off[x.row] == ((size_t)x.row < before.off.size() ? before.off[x.row] : 0));
        }
        if (rng() % 97 == 0) {  // clear: the rows go, the pool stays
            t.reset();
            CHECK(t.used == 0 && t.off.empty() && t.alloc == plan.alloc);
        }
    }
}

struct Expect {
    int row;
    long long off;
    int cap, len;
};

static void expect_rows(const RowTable& t, const std::vector<Expect>& e, long long used, long long alloc) {
    for (const Expect& x : e) {
        CHECK(t.off[x.row] == x.off);
        CHECK(t.cap[x.row] == x.cap);
        CHECK(t.len[x.row] == x.len);
    }
    CHECK(t.used == used);
    CHECK(t.alloc == alloc);
}

// The offsets map_put_rows assigned before the store existed, written out by hand from its rule:
// a row whose new length exceeds its capacity gets the next power of two >= max(4, length) at the
// pool's end, used += that; the pool goes to max(2 * alloc, 4096), doubled until it holds `used`.
static void scripted_rows() {
    RowTable t(1, 4, 4096);
    auto run = [&](std::vector<RowNeed> need) {
        const RowPlan p = t.plan(need);
        t.commit(p);
        return p;
    };
    RowPlan p = run({{0, 0, 3}, {1, 0, 5}, {2, 0, 0}, {3, 0, 4}});
    expect_rows(t, {{0, 0, 4, 3}, {1, 4, 8, 5}, {2, 0, 0, 0}, {3, 12, 4, 4}}, 16, 4096);
    CHECK(p.moves.size() == 3);
    p = run({{0, 0, 4}, {1, 0, 9}, {2, 0, 1}});
    expect_rows(t, {{0, 0, 4, 4}, {1, 16, 16, 9}, {2, 32, 4, 1}, {3, 12, 4, 4}}, 36, 4096);
    CHECK(p.moves.size() == 2 && p.moves[0].row == 1 && p.moves[1].row == 2);
    p = run({{1, 0, 2}, {5, 0, 17}, {0, 0, -1}});
    expect_rows(t, {{0, 0, 4, 4}, {1, 16, 16, 2}, {4, 0, 0, 0}, {5, 36, 32, 17}}, 68, 4096);
    CHECK(p.moves.size() == 1 && p.moves[0].new_off == 36 && p.moves[0].new_cap == 32);
    p = run({{6, 0, 5000}});
    expect_rows(t, {{6, 68, 8192, 5000}}, 8260, 16384);
    p = run({{6, 0, 8192}, {7, 0, 8125}});
    expect_rows(t, {{6, 68, 8192, 8192}, {7, 8260, 8192, 8125}}, 16452, 32768);
}

// The same for cov_reserve: a row that needs more entries than its capacity gets the next power
// of two >= max(8, entries), four arrays of it, at the pool's end; the pool goes to
// max(2 * alloc, 65536), doubled until it holds `used`.
static void scripted_graph() {
    RowTable t(4, 8, 1 << 16);
    t.cover(7);
    auto run = [&](std::vector<RowNeed> need) {
        const RowPlan p = t.plan(need);
        t.commit(p);
        return p;
    };
    RowPlan p = run({{0, 3, -1}, {1, 9, -1}});
    expect_rows(t, {{0, 0, 8, 0}, {1, 32, 16, 0}}, 96, 65536);
    p = run({{0, 8, -1}});
    CHECK(p.moves.empty());
    expect_rows(t, {{0, 0, 8, 0}}, 96, 65536);
    p = run({{0, 9, -1}, {2, 0, -1}});  // 8 -> 16 entries: a new region, the old one left behind
    expect_rows(t, {{0, 96, 16, 0}, {1, 32, 16, 0}, {2, 0, 0, 0}}, 160, 65536);
    p = run({{3, 4000, -1}, {4, 4096, -1}, {5, 4096, -1}});
    expect_rows(t, {{3, 160, 4096, 0}, {4, 16544, 4096, 0}, {5, 32928, 4096, 0}}, 49312, 65536);
    p = run({{6, 4096, -1}});  // the pool crosses its first 65,536 ints
    expect_rows(t, {{6, 49312, 4096, 0}}, 65696, 131072);
    CHECK(side_pool_plan(t, 65536).alloc == 131072 && side_pool_plan(t, 65536).keep == 65536);
}

// Capacities, covered counts and the prefix a growth copies, for the rules the handle uses:
// keyframes from max(hint, 16), points from max(hint, 1024), the graph's columns from 16.
static void column_groups() {
    ColumnGroup kf;
    kf.alloc = 16;  // hint 0
    for (int n = 1; n <= 16; ++n) {
        CHECK(kf.capacity_for(n, 16) == 16);
        kf.cover(n);
    }
    CHECK(kf.covered == 16);
    CHECK(kf.capacity_for(17, 16) == 32);  // the prefix copied is `covered`: all 16
    kf.alloc = 32;
    kf.cover(17);
    CHECK(kf.capacity_for(32, 16) == 32 && kf.capacity_for(33, 16) == 64);
    ColumnGroup hinted;
    hinted.alloc = 100;
    CHECK(hinted.capacity_for(100, 16) == 100 && hinted.capacity_for(101, 16) == 200);
    ColumnGroup mp;
    mp.alloc = 1024;
    CHECK(mp.capacity_for(1024, 1024) == 1024 && mp.capacity_for(1025, 1024) == 2048);
    CHECK(mp.capacity_for(5000, 1024) == 8192);  // one add that skips doublings
    ColumnGroup lazy;  // made by its first call: covers the map as it then is
    CHECK(lazy.capacity_for(0, 16) == 0);
    CHECK(lazy.capacity_for(1, 16) == 16 && lazy.capacity_for(40, 16) == 64);
    lazy.alloc = 64;
    lazy.cover(40);
    CHECK(lazy.covered == 40);
    lazy.cover(12);  // never shrinks: what was written stays in the prefix until a clear
    CHECK(lazy.covered == 40);
    std::mt19937 rng(5);
    ColumnGroup g;
    int n = 0;
    for (int step = 0; step < 2000; ++step) {
        n += (int)(rng() % 50);
        const int cap = g.capacity_for(n, 16);
        CHECK(cap >= n && cap >= g.alloc);
        if (cap != g.alloc) {
            CHECK(cap >= 2 * g.alloc && (cap < 2 * n || cap == 16));
            CHECK(g.covered <= g.alloc);  // the prefix copied fits the old buffers
            g.alloc = cap;
        }
        g.cover(n);
        CHECK(g.covered == n && g.covered <= g.alloc);
        if (rng() % 211 == 0) n = g.covered = 0;  // clear
    }
}

int main() {
    scripted_rows();
    scripted_graph();
    column_groups();
    for (unsigned seed = 1; seed <= 6; ++seed) {
        random_run(1, 4, 4096, seed, 400);
        random_run(4, 8, 1 << 16, 100 + seed, 400);
    }
    if (g_failed) {
        std::printf("%d checks failed\n", g_failed);
        return 1;
    }
    std::printf("map_store_plan_test ok\n");
    return 0;
}
