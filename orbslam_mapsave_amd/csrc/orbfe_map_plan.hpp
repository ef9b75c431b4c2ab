// orbfe_map_plan.hpp — the arithmetic under the device map's store (orbfe_map_store.hip): where the
// rows of a ragged table lie, what a batch of row changes moves, what a pool or a group of columns
// must grow to and which prefix of it survives.  Host bookkeeping only: nothing here touches the
// device, so tests/cpp/map_store_plan_test.cpp drives it alone, under sanitizers.
#pragma once

#include <algorithm>
#include <cstddef>
#include <vector>

namespace orbfe {

// Per-keyframe or per-point arrays that grow together.  Elements [0, covered) may hold data;
// every element at or past `covered` holds its column's default (the store fills a buffer when it
// allocates it and refills [0, covered) on clear), so covering more elements is bookkeeping.
struct ColumnGroup {
    int alloc = 0;    // elements every column of the group holds
    int covered = 0;  // elements that may differ from the default: the prefix a growth copies

    // The capacity that holds n elements: unchanged while they fit, else doubled from
    // max(2 * alloc, start) until they do.
    int capacity_for(int n, int start) const {
        if (n <= alloc) return alloc;
        int a = std::max(2 * alloc, start);
        while (a < n) a *= 2;
        return a;
    }
    void cover(int n) { covered = std::max(covered, n); }
};

struct RowNeed {
    int row;
    int entries;  // the region must hold at least this many
    int new_len;  // the row's length afterwards, or -1: unchanged
};

struct RowMove {
    int row;
    long long new_off;
    int new_cap;
};

struct RowPlan {
    std::vector<RowMove> moves;  // the rows that get a new region, in the order of the batch
    long long used = 0;          // the pool's used ints afterwards
    long long alloc = 0;         // what the pool must grow to (the table's `alloc`: no growth)
};

// Rows of `lanes` arrays of cap ints each, in one pool: row r is at [off[r], off[r] + lanes * cap[r]).
// A row that outgrows its region gets a new one of a power of two entries (at least `min_cap`) at
// the pool's end; the old region is not reused, so the pool holds at most twice what the rows do.
// The pool doubles from `first_alloc` ints.
struct RowTable {
    int lanes, min_cap;
    long long first_alloc;
    std::vector<long long> off;
    std::vector<int> cap, len;
    long long used = 0, alloc = 0;

    RowTable(int lanes_, int min_cap_, long long first_alloc_)
        : lanes(lanes_), min_cap(min_cap_), first_alloc(first_alloc_) {}

    void reset() {  // the pool stays
        off.clear();
        cap.clear();
        len.clear();
        used = 0;
    }
    void cover(size_t rows) {  // new rows: no region, length 0
        if (off.size() >= rows) return;
        off.resize(rows, 0);
        cap.resize(rows, 0);
        len.resize(rows, 0);
    }
    int length(int row) const { return (size_t)row < len.size() ? len[row] : 0; }

    // Plans the batch in order and records the rows' new (off, cap, len) here; `used` and `alloc`
    // stay until commit(), so the caller grows the pool from the old extent first.
    RowPlan plan(const std::vector<RowNeed>& need) {
        RowPlan p;
        p.used = used;
        for (const RowNeed& x : need) {
            cover((size_t)x.row + 1);
            const int n = x.new_len >= 0 ? x.new_len : len[x.row];
            const int entries = std::max(x.entries, n);
            if (entries > cap[x.row]) {
                int c = min_cap;
                while (c < entries) c <<= 1;
                off[x.row] = p.used;
                cap[x.row] = c;
                p.moves.push_back({x.row, p.used, c});
                p.used += (long long)lanes * c;
            }
            len[x.row] = n;
        }
        p.alloc = alloc;
        if (p.used > alloc) {
            p.alloc = std::max(2 * alloc, first_alloc);
            while (p.alloc < p.used) p.alloc *= 2;
        }
        return p;
    }
    void commit(const RowPlan& p) {
        used = p.used;
        alloc = p.alloc;
    }
};

// A pool that shares a table's offsets and grows with it: what it must hold, and the prefix that
// may differ from its default (what a growth copies and a clear refills).
struct SidePoolPlan {
    long long alloc, keep;
};
inline SidePoolPlan side_pool_plan(const RowTable& t, long long side_alloc) {
    return {t.alloc, std::min(t.used, side_alloc)};
}

}  // namespace orbfe
