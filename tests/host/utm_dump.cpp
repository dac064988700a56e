// Runs the functions of csrc/satba_utm_geom.h and csrc/satba_elbow.h on the host and dumps what they compute (tests/test_utm_host.py).
// argv[1]: a file of float64; stdout: float64
//   mode 0  filter:   [0, margin, n_pairs, pair_ofs (n_pairs + 1), utm (4 n), alive (n)] -> keep (n), thr (n_pairs), n_kept (n_pairs):
//                     the rule of satba_utm_filter, sequentially: utm_distance, a sort, elbow_sequential, the kernel's last step
//   mode 1  project:  [1, n, (lon, lat, zone) x n] -> (east, north) x n
//   mode 2  zone:     [2, n, lon x n] -> zone x n
//   mode 3  elbow:    [3, n, v (n, ascending)] -> elbow, success, v[n - 1]
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "satba_elbow.h"
#include "satba_utm_geom.h"

static void put(const std::vector<double>& v) {
    if (!v.empty()) fwrite(v.data(), sizeof(double), v.size(), stdout);
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<double> in;
    double buf[1024];
    size_t got;
    while ((got = fread(buf, sizeof(double), 1024, f)) > 0) in.insert(in.end(), buf, buf + got);
    fclose(f);
    if (in.size() < 2) return 2;
    const int mode = (int)in[0];
    std::vector<double> out;
    if (mode == 0) {
        if (in.size() < 4) return 2;
        const double margin = in[1];
        const size_t n_pairs = (size_t)in[2];
        if (in.size() < 3 + n_pairs + 1) return 2;
        const double* ofs = in.data() + 3;
        const size_t n = (size_t)ofs[n_pairs];
        if (in.size() != 3 + n_pairs + 1 + 5 * n) return 2;
        const double* utm = ofs + n_pairs + 1;
        const double* alive = utm + 4 * n;
        std::vector<double> keep(n, 0.0), thr(n_pairs), kept(n_pairs, 0.0), d(n);
        for (size_t i = 0; i < n; ++i) d[i] = alive[i] != 0.0 ? utm_distance(utm + 4 * i) : 0.0;
        for (size_t p = 0; p < n_pairs; ++p) {
            const size_t a = (size_t)ofs[p], b = (size_t)ofs[p + 1];
            std::vector<double> v;
            for (size_t i = a; i < b; ++i)
                if (alive[i] != 0.0) v.push_back(d[i]);
            std::sort(v.begin(), v.end());
            thr[p] = v.empty() ? std::nan("") : utm_threshold(satba::elbow_sequential(v.data(), (int)v.size()), margin);
            for (size_t i = a; i < b; ++i)
                if (alive[i] != 0.0 && d[i] <= thr[p]) { keep[i] = 1.0; kept[p] += 1.0; }
        }
        put(keep); put(thr); put(kept);
    } else if (mode == 1) {
        const size_t n = (size_t)in[1];
        if (in.size() != 2 + 3 * n) return 2;
        for (size_t i = 0; i < n; ++i) {
            double e, nn;
            utm_project(in[2 + 3 * i], in[3 + 3 * i], (int)in[4 + 3 * i], e, nn);
            out.push_back(e); out.push_back(nn);
        }
        put(out);
    } else if (mode == 2) {
        const size_t n = (size_t)in[1];
        if (in.size() != 2 + n) return 2;
        for (size_t i = 0; i < n; ++i) out.push_back((double)utm_zone(in[2 + i]));
        put(out);
    } else if (mode == 3) {
        const size_t n = (size_t)in[1];
        if (n < 1 || in.size() != 2 + n) return 2;
        const satba::Elbow e = satba::elbow_sequential(in.data() + 2, (int)n);
        out = {e.elbow, e.success ? 1.0 : 0.0, e.last};
        put(out);
    } else {
        return 2;
    }
    return 0;
}
