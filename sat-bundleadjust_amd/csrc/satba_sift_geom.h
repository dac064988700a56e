// Geometry of the SIFT scale space: octave count, plane sizes, sigmas, blur increments and the normalised
// tap tables.  Plain C++ that compiles on the host on its own (tests/host/sift_geom_dump.cpp); the launcher of the kernels in
// satba_sift.h reads the same tables.  The rules are those of "Anatomy of the SIFT method" as the reference's SIMD library runs
// them (ref:3rdparty/sift/simd/LibSift/ScaleSpace.cpp:82-98, LibSift.cpp:210-283, LibImages/LibImages.cpp:383-395), with every
// intermediate in the number format the reference uses, so that a table here equals the reference's float for float.
#pragma once
#include <cmath>
#include <cstdint>

constexpr int SIFT_MAX_OCT = 24;     // 2 * side / 12 < 2^24 for any side an int32 holds a plane of
constexpr int SIFT_MAX_SCALES = 13;  // nb_scales; planes per octave = nb_scales + 3 <= SIFT_MAX_PLANES
constexpr int SIFT_MAX_PLANES = SIFT_MAX_SCALES + 3;
constexpr int SIFT_MAX_RADIUS = 32;  // taps kept per blur: ceil(4 sigma) <= 32 (13 at the defaults)
constexpr float SIFT_DELTA_MIN = 0.5f, SIFT_SIGMA_MIN = 0.8f, SIFT_SIGMA_IN = 0.5f;

struct SiftGeom {
    int32_t n_oct, n_planes;  // planes per octave (Gaussian); DoG planes = n_planes - 1, searched scales 1 .. n_planes - 3
    int32_t w[SIFT_MAX_OCT], h[SIFT_MAX_OCT];
    float delta[SIFT_MAX_OCT];
    float sigma[SIFT_MAX_OCT][SIFT_MAX_PLANES];
    float inc[SIFT_MAX_OCT][SIFT_MAX_PLANES];  // blur that makes plane s: from the seed (o = 0, s = 0), nothing (o > 0, s = 0), from plane s - 1
    float thr;                                 // the DoG threshold converted to nb_scales
};

// min(nb_octaves, floor(log2(h0 / 12)) + 1), h0 = min(w, h) / delta_min; h0 / 12 is an integer division
inline int sift_octave_count(int w, int h, int nb_octaves) {
    const size_t h0 = (size_t)((float)(w < h ? w : h) / SIFT_DELTA_MIN);
    const size_t q = h0 / 12;
    if (q < 1) return 0;
    const int n = (int)(size_t)(std::log((double)q) / M_LN2) + 1;
    return nb_octaves < n ? nb_octaves : n;
}

inline float sift_threshold(float thresh_dog, int nb_scales) {
    const float k_nspo = (float)std::exp(M_LN2 / (double)(float)nb_scales);
    const float k_3 = (float)std::exp(M_LN2 / (double)(float)3);
    return (k_nspo - 1) / (k_3 - 1) * thresh_dog;
}

// returns 0, or -1 when the sizes leave no octave / more scales than the tables hold
inline int sift_geometry(int w, int h, int nb_octaves, int nb_scales, float thresh_dog, SiftGeom* g) {
    if (nb_scales < 1 || nb_scales > SIFT_MAX_SCALES) return -1;
    int n = sift_octave_count(w, h, nb_octaves);
    if (n < 1) return -1;
    if (n > SIFT_MAX_OCT) n = SIFT_MAX_OCT;
    g->n_oct = n;
    g->n_planes = nb_scales + 3;
    g->thr = sift_threshold(thresh_dog, nb_scales);
    const size_t h0 = (size_t)((float)h / SIFT_DELTA_MIN), w0 = (size_t)((float)w / SIFT_DELTA_MIN);
    for (int o = 0; o < n; ++o) {
        const float dn = SIFT_DELTA_MIN * (float)(1 << o);
        g->delta[o] = dn;
        g->h[o] = (int32_t)(h0 / ((size_t)1 << o));
        g->w[o] = (int32_t)(w0 / ((size_t)1 << o));
        for (int s = 0; s < g->n_planes; ++s)
            g->sigma[o][s] = (float)((double)(dn / SIFT_DELTA_MIN * SIFT_SIGMA_MIN) * std::pow(2.0, (double)((float)s / (float)nb_scales)));
        for (int s = 0; s < SIFT_MAX_PLANES; ++s) g->inc[o][s] = 0.0f;
        for (int s = 1; s < g->n_planes; ++s) {
            const float sp = g->sigma[o][s - 1], sn = g->sigma[o][s];
            const float a = sn * sn, b = sp * sp;  // rounded one by one: no fused multiply-add
            g->inc[o][s] = std::sqrt(a - b) / dn;
        }
    }
    const float s0 = g->sigma[0][0];
    const float a = s0 * s0, b = SIFT_SIGMA_IN * SIFT_SIGMA_IN;
    g->inc[0][0] = std::sqrt(a - b) / SIFT_DELTA_MIN;
    return 0;
}

inline int sift_radius(float sigma) { return (int)std::ceil(4 * sigma); }

// normalised taps ker[0 .. radius] of a blur by sigma; returns the radius, or -1 when it exceeds SIFT_MAX_RADIUS
inline int sift_taps(float sigma, float* ker) {
    const int r = sift_radius(sigma);
    if (r > SIFT_MAX_RADIUS) return -1;
    ker[0] = 1.0f;
    if (sigma > 0) {
        float sum = ker[0];
        for (int k = 1; k <= r; ++k) {
            ker[k] = (float)std::exp(-0.5 * (double)(float)k * (double)(float)k / (double)sigma / (double)sigma);
            const float two = 2 * ker[k];
            sum = sum + two;
        }
        for (int k = 0; k <= r; ++k) ker[k] = ker[k] / sum;
    } else {
        for (int k = 1; k <= r; ++k) ker[k] = 0.0f;
    }
    return r;
}
