// Runs the functions of csrc/satba_ransac_geom.h on the host and dumps what they compute (tests/test_ransac_host.py).
// argv[1]: a file of float64 = [mode, seed low 32 bits, seed high 32 bits, p, n_trials, max_err, m, n_extra, xy (4 m), extra ...]
// stdout: float64
//   mode 0  draws:   per trial t < n_trials: found (0 / 1), the seven indices
//   mode 1  models:  extra = n_extra samples x 7 indices -> per sample: n_models, 3 x 9 matrix entries (zeros behind the models)
//   mode 2  errors:  extra = n_extra matrices x 9 -> per matrix the m errors
//   mode 3  ransac:  the whole rule for pair p: live (0 / 1); per trial: n_models, 3 x (count, sum) (-1, 0: no model); then the
//                    winner: trial, count, models of the pair, 9 matrix entries, m mask values
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "satba_ransac_geom.h"

static void put(const std::vector<double>& v) { fwrite(v.data(), sizeof(double), v.size(), stdout); }

static bool models_of(const double* xy, const int64_t* idx, const double* T, RscModels* out) {
    RscRows rows;
    for (int j = 0; j < 7; ++j)
        for (int e = 0; e < 4; ++e) rows.v[j][e] = xy[4 * idx[j] + e];
    out->n = 0;
    if (rsc_rows_repeat(rows)) return false;
    rsc_seven_point(rows, T, out);
    return true;
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
    if (in.size() < 8) return 2;
    const int mode = (int)in[0];
    const uint64_t seed = (uint64_t)in[1] | ((uint64_t)in[2] << 32);
    const uint64_t p = (uint64_t)in[3], n_trials = (uint64_t)in[4];
    const double max_err = in[5], thr2 = max_err * max_err;
    const int64_t m = (int64_t)in[6], n_extra = (int64_t)in[7];
    if (in.size() < 8 + 4 * (size_t)m) return 2;
    const double* xy = in.data() + 8;
    const double* extra = xy + 4 * m;
    const size_t n_rest = in.size() - 8 - 4 * (size_t)m;
    std::vector<double> out;
    double T[6] = {0, 0, 0, 0, 0, 0};
    const bool live = m >= RSC_MIN_MATCHES && rsc_normalise(xy, m, T);
    if (mode == 0) {
        for (uint64_t t = 0; t < n_trials; ++t) {
            RscSample s;
            out.push_back(rsc_sample(seed, p, n_trials, t, (uint64_t)m, &s) ? 1.0 : 0.0);
            for (int j = 0; j < 7; ++j) out.push_back((double)s.i[j]);
        }
    } else if (mode == 1) {
        if (n_rest < 7 * (size_t)n_extra) return 2;
        const bool have_T = rsc_normalise(xy, m, T);
        for (int64_t g = 0; g < n_extra; ++g) {
            int64_t idx[7];
            for (int j = 0; j < 7; ++j) {
                idx[j] = (int64_t)extra[7 * g + j];
                if (idx[j] < 0 || idx[j] >= m) return 2;
            }
            RscModels mo;
            mo.n = 0;
            if (have_T) models_of(xy, idx, T, &mo);
            out.push_back((double)mo.n);
            for (int r = 0; r < 3; ++r)
                for (int k = 0; k < 9; ++k) out.push_back(r < mo.n ? mo.F[r][k] : 0.0);
        }
    } else if (mode == 2) {
        if (n_rest < 9 * (size_t)n_extra) return 2;
        for (int64_t g = 0; g < n_extra; ++g)
            for (int64_t i = 0; i < m; ++i) out.push_back(rsc_error(extra + 9 * g, xy[4 * i], xy[4 * i + 1], xy[4 * i + 2], xy[4 * i + 3]));
    } else if (mode == 3) {
        out.push_back(live ? 1.0 : 0.0);
        int best_cnt = -1, best_trial = -1, n_models = 0;
        double best_sum = 0.0, best_F[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        for (uint64_t t = 0; t < n_trials; ++t) {
            RscModels mo;
            mo.n = 0;
            RscSample s;
            if (live && rsc_sample(seed, p, n_trials, t, (uint64_t)m, &s)) models_of(xy, s.i, T, &mo);
            out.push_back((double)mo.n);
            n_models += mo.n;
            for (int r = 0; r < 3; ++r) {
                if (r >= mo.n) {
                    out.push_back(-1.0);
                    out.push_back(0.0);
                    continue;
                }
                int cnt = 0;
                double sum = 0.0;
                for (int64_t i = 0; i < m; ++i) {
                    const double e = rsc_error(mo.F[r], xy[4 * i], xy[4 * i + 1], xy[4 * i + 2], xy[4 * i + 3]);
                    if (e < thr2) { ++cnt; sum += e; }
                }
                out.push_back((double)cnt);
                out.push_back(sum);
                // trials ascend, so a later trial wins only with more inliers; inside a trial the smaller sum, then the first root
                if (cnt > best_cnt || (cnt == best_cnt && best_trial == (int)t && sum < best_sum)) {
                    best_cnt = cnt; best_trial = (int)t; best_sum = sum;
                    for (int k = 0; k < 9; ++k) best_F[k] = mo.F[r][k];
                }
            }
        }
        out.push_back((double)best_trial);
        out.push_back(best_cnt >= 0 ? (double)best_cnt : (double)m);
        out.push_back((double)n_models);
        for (int k = 0; k < 9; ++k) out.push_back(best_F[k]);
        for (int64_t i = 0; i < m; ++i)
            out.push_back(best_cnt < 0 || rsc_error(best_F, xy[4 * i], xy[4 * i + 1], xy[4 * i + 2], xy[4 * i + 3]) < thr2 ? 1.0 : 0.0);
    } else {
        return 2;
    }
    put(out);
    return 0;
}
