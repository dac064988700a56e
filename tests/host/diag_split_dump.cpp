// Prints the split camera c* of the diagonal pass (csrc/satba_diag_split.h) for every number of late tile columns 0 .. T + 1, one
// line each: "late_cols c* T", then the forced splits "from <camera> c*" and the default number of late columns "default <cols>".   usage: diag_split_dump M NP [applies = 1]
#include <cstdio>
#include <cstdlib>

#include "satba_diag_split.h"

int main(int argc, char** argv) {
    if (argc != 3 && argc != 4) {
        fprintf(stderr, "usage: %s M NP [applies]\n", argv[0]);
        return 2;
    }
    const int M = atoi(argv[1]), NP = atoi(argv[2]);
    const bool applies = argc == 4 ? atoi(argv[3]) != 0 : true;
    const int T = satba::diag_split_tiles(M, NP);
    for (int late = 0; late <= T + 1; ++late) printf("%d %d %d\n", late, satba::diag_split_camera(M, NP, late, applies), T);
    for (int from = -1; from <= M + 1; ++from) printf("from %d %d\n", from, satba::diag_split_forced(M, from, applies));
    printf("default %d\n", satba::diag_late_cols_default(T));
    return 0;
}
