// Writes one item table of k_schur_pairs (csrc/satba_schur_items.h) to stdout as raw int32 pairs (pair, chunk) in dispatch order.
// usage: schur_items_dump kind M C spc dg_weight   (kind: 0 chunked, 1 merged, 2 weighted)
#include <cstdio>
#include <cstdlib>

#include "satba_schur_items.h"

int main(int argc, char** argv) {
    if (argc != 6) {
        fprintf(stderr, "usage: %s kind M C spc dg_weight\n", argv[0]);
        return 2;
    }
    const int kind = atoi(argv[1]);
    if (kind < 0 || kind > 2) return 2;
    const std::vector<satba::SchurItemKey> table =
        satba::schur_item_order(static_cast<satba::SchurTable>(kind), atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atoll(argv[5]));
    static_assert(sizeof(satba::SchurItemKey) == 2 * sizeof(int), "raw int32 pairs");
    return fwrite(table.data(), sizeof(satba::SchurItemKey), table.size(), stdout) == table.size() ? 0 : 1;
}
