// The scalar side of the trust-region loop (csrc/satba_lm.h) as a host compiler builds it, on rows of float64 read from stdin and
// written to stdout as raw bytes.   usage: lm_scalars_dump rows | radius | term
//   rows    a b c g0 g1 Delta                              -> p0 p1 newton Delta_new ratio term   (satba_lm::lm_scalars_row)
//   radius  Delta actual predicted step_norm bound_hit     -> Delta_new ratio                     (update_tr_radius)
//   term    dF F dx_norm x_norm ratio ftol xtol            -> term                                (check_termination)
#include <cstdio>
#include <cstring>
#include <vector>

#include "satba_lm.h"

int main(int argc, char** argv) {
    const char* mode = argc == 2 ? argv[1] : "";
    const int n_in = !strcmp(mode, "rows") ? 6 : !strcmp(mode, "radius") ? 5 : !strcmp(mode, "term") ? 7 : 0;
    if (!n_in) {
        fprintf(stderr, "usage: %s rows|radius|term < float64 rows > float64 rows\n", argv[0]);
        return 2;
    }
    std::vector<double> in;
    double buf[4096];
    size_t got;
    while ((got = fread(buf, sizeof(double), 4096, stdin)) > 0) in.insert(in.end(), buf, buf + got);
    if (in.size() % n_in) {
        fprintf(stderr, "%zu values are no whole number of rows of %d\n", in.size(), n_in);
        return 2;
    }
    const size_t n = in.size() / n_in;
    const int n_out = n_in == 6 ? 6 : n_in == 5 ? 2 : 1;
    std::vector<double> out(n * n_out);
    for (size_t i = 0; i < n; ++i) {
        const double* r = &in[i * n_in];
        double* o = &out[i * n_out];
        if (n_in == 6) satba_lm::lm_scalars_row(r, o);
        else if (n_in == 5) o[0] = satba_lm::update_tr_radius(r[0], r[1], r[2], r[3], r[4] != 0.0, o[1]);
        else o[0] = (double)satba_lm::check_termination(r[0], r[1], r[2], r[3], r[4], r[5], r[6]);
    }
    if (!out.empty() && fwrite(out.data(), sizeof(double), out.size(), stdout) != out.size()) return 1;
    return 0;
}
