// satba_schur_items.h -- dispatch order of the work items of k_schur_pairs (satba_schur.h).  Plain C++, no HIP: a host program can
// check the order without a device (tests/host/schur_items_dump.cpp).
#pragma once
#include <algorithm>
#include <vector>

namespace satba {
// chunked: one item per (pair, point-range chunk).
// merged: one item per pair covering all its chunks (chunk = -1 in the table): the unit-weight kernels gather nothing per
// observation and are faster with four times fewer, longer items (0.548 vs 0.576 ms at 200 x 1M x 10M) -- the weighted / robust
// kernels are not (their row-scale gathers want the locality of the point-range chunks: 1.58 vs 1.74 ms with two chunks).
// weighted: the chunked items of the weighted / robust pair kernel on the merged records, with the diagonal items of
// (camera i, chunk) -- spc of them, one wave each over an equal share of the camera's entries in the chunk -- in FRONT of the
// pair items (i, j > i) of that chunk: they pull the chunk's records of camera i into the XCD's L2, where the pair items then
// find them.  The last camera has no pair items: its diagonal items form groups of their own.
enum SchurTable { SCHUR_ITEMS_CHUNKED, SCHUR_ITEMS_MERGED, SCHUR_ITEMS_WEIGHTED };
// pair >= 0: pair item (pair_index of satba_layout.h; chunk -1: all chunks) | -1: padding | <= -2: diagonal item of camera -2 - pair, `chunk` its slot
struct SchurItemKey { int pair, chunk; };

// The rows of the pair triangle (all pairs (i, j > i) of one camera i) are dealt to the 8 XCDs longest-first onto the least loaded
// one (dg_weight: what a row's diagonal items weigh, in pair items); an XCD's items are ordered row by row, chunk by chunk, every
// (row, chunk) group padded to whole workgroups of 4 items; workgroup b = 8 s + x takes the s-th group of 4 items of XCD x.
// Beside the factorisation two waits lean on this order (the item of a pair's last chunk adds up the others' partials, the last
// diagonal item of a camera the others': every other one has been started before it), and the rows of an XCD ascend, so that the
// columns of S are finished from the left.  tests/test_schur_items_host.py holds the order to that.
inline std::vector<SchurItemKey> schur_item_order(SchurTable kind, int M, int C, int spc, long long dg_weight) {
    constexpr int X = 8;
    const bool weighted = kind == SCHUR_ITEMS_WEIGHTED, merged = kind == SCHUR_ITEMS_MERGED;
    const SchurItemKey pad{-1, 0};
    std::vector<std::vector<SchurItemKey>> per(X);
    std::vector<long long> load(X, 0);
    for (int i = 0; i + (weighted ? 0 : 1) < M; ++i) {  // rows by decreasing length: i ascending
        int x = 0;
        for (int k = 1; k < X; ++k) if (load[k] < load[x]) x = k;
        load[x] += (M - 1 - i) + (weighted ? dg_weight : 0);
        const long long first = (long long)i * M - (long long)i * (i + 1) / 2;  // pair_index(M, i, i + 1)
        for (int ch = 0; ch < (merged ? 1 : C); ++ch) {
            if (weighted) for (int sub = 0; sub < spc; ++sub) per[x].push_back({-2 - i, ch * spc + sub});
            for (int j = i + 1; j < M; ++j) per[x].push_back({(int)(first + j - i - 1), merged ? -1 : ch});
            while (per[x].size() % 4) per[x].push_back(pad);  // a workgroup stays inside one (row, chunk) group
        }
    }
    size_t slots = 0;
    for (int x = 0; x < X; ++x) slots = std::max(slots, per[x].size() / 4);
    if (slots == 0) return std::vector<SchurItemKey>(4, pad);
    std::vector<SchurItemKey> table(slots * X * 4, pad);
    for (int x = 0; x < X; ++x)
        for (size_t s = 0; s < per[x].size() / 4; ++s)
            for (int w = 0; w < 4; ++w) table[(s * X + x) * 4 + w] = per[x][s * 4 + w];
    return table;
}
}  // namespace satba
