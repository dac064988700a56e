// Runs the functions of csrc/satba_window_cells.h on the host and dumps what they compute (tests/test_window_host.py).
// argv[1]: a file of float64 [rx, ry, n_j, n_i, (east, north) x n_j, (east, north) x n_i]: the selected keypoints of a pair's second
// side, which the grid is laid over as k_window_grid does, and the queries.
// stdout: float64 [x.o, x.w, x.n, y.o, y.w, y.n, (cell_x, cell_y) x n_j, (cx0, cx1, cy0, cy1) x n_i]
#include <cmath>
#include <cstdio>
#include <vector>

#include "satba_window_cells.h"

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<double> in;
    double buf[1024];
    size_t got;
    while ((got = fread(buf, sizeof(double), 1024, f)) > 0) in.insert(in.end(), buf, buf + got);
    fclose(f);
    if (in.size() < 4) return 2;
    const double rx = in[0], ry = in[1];
    const size_t n_j = (size_t)in[2], n_i = (size_t)in[3];
    if (in.size() != 4 + 2 * n_j + 2 * n_i) return 2;
    const double* uj = in.data() + 4;
    const double* ui = uj + 2 * n_j;
    double e0 = INFINITY, e1 = -INFINITY, n0 = INFINITY, n1 = -INFINITY;
    for (size_t k = 0; k < n_j; ++k) {
        e0 = std::fmin(e0, uj[2 * k]); e1 = std::fmax(e1, uj[2 * k]);
        n0 = std::fmin(n0, uj[2 * k + 1]); n1 = std::fmax(n1, uj[2 * k + 1]);
    }
    WcGrid g;
    g.x = wc_axis(e0, e1, rx);
    g.y = wc_axis(n0, n1, ry);
    std::vector<double> out = {g.x.o, g.x.w, (double)g.x.n, g.y.o, g.y.w, (double)g.y.n};
    for (size_t k = 0; k < n_j; ++k) {
        out.push_back((double)wc_cell(g.x, uj[2 * k]));
        out.push_back((double)wc_cell(g.y, uj[2 * k + 1]));
    }
    for (size_t k = 0; k < n_i; ++k) {
        int c0, c1, r0, r1;
        wc_range(g.x, ui[2 * k], rx, c0, c1);
        wc_range(g.y, ui[2 * k + 1], ry, r0, r1);
        // the key the sort orders by must keep (cell_y, cell_x) apart
        if (wc_key(1, r1, c1) >> (2 * WC_DIM_BITS) != 1 || (wc_key(0, r0, c0) & (WC_MAX_DIM - 1)) != (uint64_t)c0) return 3;
        out.push_back((double)c0); out.push_back((double)c1); out.push_back((double)r0); out.push_back((double)r1);
    }
    fwrite(out.data(), sizeof(double), out.size(), stdout);
    return 0;
}
