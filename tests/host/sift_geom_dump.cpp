// Dumps the SIFT scale-space geometry of csrc/satba_sift_geom.h for tests/test_sift_host.py, which compares it with the restatement
// in tests/cases_sift.py.  Host only: the header is plain C++.
//   sift_geom_dump <width> <height> <nb_octaves> <nb_scales> <thresh_dog>
// writes to stdout, as 32-bit words: n_oct, n_planes, thr (float), then per octave w, h, delta (float), n_planes sigmas (float),
// n_planes increments (float), and per increment its radius and radius + 1 taps (float).  Exit code 2: no octave fits.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "satba_sift_geom.h"

static std::vector<int32_t> out;
static void put_i(int32_t v) { out.push_back(v); }
static void put_f(float f) {
    int32_t v;
    memcpy(&v, &f, sizeof v);
    out.push_back(v);
}

int main(int argc, char** argv) {
    if (argc != 6) {
        fprintf(stderr, "usage: %s width height nb_octaves nb_scales thresh_dog\n", argv[0]);
        return 1;
    }
    SiftGeom g;
    if (sift_geometry(atoi(argv[1]), atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), (float)atof(argv[5]), &g)) return 2;
    put_i(g.n_oct);
    put_i(g.n_planes);
    put_f(g.thr);
    for (int o = 0; o < g.n_oct; ++o) {
        put_i(g.w[o]);
        put_i(g.h[o]);
        put_f(g.delta[o]);
        for (int s = 0; s < g.n_planes; ++s) put_f(g.sigma[o][s]);
        for (int s = 0; s < g.n_planes; ++s) put_f(g.inc[o][s]);
        for (int s = 0; s < g.n_planes; ++s) {
            float ker[SIFT_MAX_RADIUS + 1];
            const int r = sift_taps(g.inc[o][s], ker);
            put_i(r);
            for (int k = 0; k <= r; ++k) put_f(ker[k]);
        }
    }
    fwrite(out.data(), sizeof(int32_t), out.size(), stdout);
    return 0;
}
