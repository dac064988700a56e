// SIFT detection and description on the device: "Anatomy of the SIFT method" as the reference's SIMD library
// runs it (ref:3rdparty/sift/simd/LibSift/*, LibImages/LibImages.cpp), restated.  Launcher: satba_sift_api.inc; geometry and tap
// tables: satba_sift_geom.h.
//
//   k_sift_seed       image / 256, 2x bilinear oversample with the reference's symmetrisation; max |pixel| for the fixed-point scale
//   k_sift_blur_cols  vertical pass of a blur over an LDS tile; k_sift_blur_rows the horizontal pass.  Sums in the reference's
//                     order with __fmul_rn / __fadd_rn (no contraction): the planes differ from a float64 restatement by float32 rounding only
//   k_sift_subsample  every second sample of a plane
//   k_sift_extrema    strict 26-neighbour extrema of the DoG (formed from four Gaussian planes where it is read) above 0.8 thr,
//                     emitted as 64-bit keys (octave, scale, row, column); a radix sort of the keys is the reference's list order
//   k_sift_refine     one lane per candidate: interpolation, both discards, the edge test, the border test
//   k_sift_orient     one wave per candidate: 36-bin histogram in the LDS, smoothing, principal orientations
//   k_sift_describe   one wave per candidate, once per orientation: 4 x 4 x 8 bins in the LDS, threshold, renormalise, quantise
//
// Histogram sums are 64-bit fixed-point LDS atomics (integer adds commute): two calls return identical bytes.  The scale of the
// fixed point comes from max |pixel| (satba_sift_api.inc): a vote is below 4 max|pixel| / 256 and a histogram has fewer than 2^14 samples.
#pragma once
#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>
#include <stdint.h>

#include "satba_sift_geom.h"

constexpr int SIFT_ORI_BINS = 36, SIFT_NHIST = 4, SIFT_NORI = 8, SIFT_DESC = SIFT_NHIST * SIFT_NHIST * SIFT_NORI, SIFT_ROW = 4 + SIFT_DESC;
constexpr int SIFT_MAX_ORI = SIFT_ORI_BINS / 2;  // strict local maxima of a circular histogram of 36 bins
constexpr int SIFT_MAX_ITER = 5;
constexpr float SIFT_OFF_MAX = 0.6f, SIFT_EDGE = 10.0f, SIFT_LAMBDA_ORI = 1.5f, SIFT_LAMBDA_DES = 6.0f, SIFT_T = 0.8f;
constexpr int SIFT_BLUR_TW = 64, SIFT_BLUR_TH = 64, SIFT_BLUR_ROWS_PER_PASS = 4, SIFT_BLUR_LINE = 256;
constexpr float SIFT_2PI = 6.283185307179586f;  // (float)(2 pi), as the reference's float modulus sees it

struct SiftTaps {
    int radius;
    float ker[SIFT_MAX_RADIUS + 1];
};

// what the kernels need of SiftGeom, with the planes' addresses: plane s of octave o is base[o] + s * w[o] * h[o]
struct SiftPlanes {
    int32_t n_oct, n_planes, img_w, img_h;
    float thr, sigma_ratio;
    float* base[SIFT_MAX_OCT];
    int32_t w[SIFT_MAX_OCT], h[SIFT_MAX_OCT];
    float delta[SIFT_MAX_OCT];
    float sigma[SIFT_MAX_OCT][SIFT_MAX_PLANES];
};

struct SiftKey {  // a candidate after k_sift_refine
    float x, y, sigma;  // x the row, y the column, in image pixels
    int32_t o, s, alive;
};

// key of a discrete extremum: octave (5 bits), scale (5), row (27), column (27)
__host__ __device__ inline unsigned long long sift_key(int o, int s, int i, int j) {
    return ((unsigned long long)o << 59) | ((unsigned long long)s << 54) | ((unsigned long long)i << 27) | (unsigned long long)j;
}

// half-sample symmetric extension (... b a | a b ...), periodic where the side is shorter than the reach
__device__ inline int sift_mirror(int m, int n) {
    const int p = 2 * n;
    m %= p;
    if (m < 0) m += p;
    return m < n ? m : p - 1 - m;
}

// ------------------------------------------------------------------------------------------------ seed
__global__ void __launch_bounds__(256) k_sift_seed(const float* __restrict__ img, long long stride, int wi, int hi, float* __restrict__ out, int wo,
                                                    int ho, unsigned* __restrict__ max_bits) {
    __shared__ unsigned s_max;
    if (threadIdx.x == 0) s_max = 0u;
    __syncthreads();
    const long long n = (long long)wo * ho, t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n) {
        const int i = (int)(t / wo), j = (int)(t % wo);
        const float x = i * SIFT_DELTA_MIN, y = j * SIFT_DELTA_MIN;
        const int dx = (int)x, dy = (int)y;
        const int im = dx >= hi ? 2 * hi - 1 - dx : dx, ip = dx + 1 >= hi ? 2 * hi - 1 - dx - 1 : dx + 1;
        const int jm = dy >= wi ? 2 * wi - 1 - dy : dy, jp = dy + 1 >= wi ? 2 * wi - 1 - dy - 1 : dy + 1;
        const float fx = x - floorf(x), fy = y - floorf(y);
        const float c = 1.0f / 256.0f;
        const float pp = img[ip * stride + jp] * c, pm = img[ip * stride + jm] * c, mp = img[im * stride + jp] * c, mm = img[im * stride + jm] * c;
        const float a = __fadd_rn(__fmul_rn(fy, pp), __fmul_rn(1.0f - fy, pm)), b = __fadd_rn(__fmul_rn(fy, mp), __fmul_rn(1.0f - fy, mm));
        out[t] = __fadd_rn(__fmul_rn(fx, a), __fmul_rn(1.0f - fx, b));
        // |v| as bits orders like |v|; a NaN or an infinity is >= 0x7f800000
        const unsigned bits = __float_as_uint(mm) & 0x7fffffffu;
        atomicMax(&s_max, bits);
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_max) atomicMax(max_bits, s_max);
}

// ------------------------------------------------------------------------------------------------ blur
// vertical pass: tile of SIFT_BLUR_TH rows x SIFT_BLUR_TW columns, halo of `radius` rows above and below
__global__ void __launch_bounds__(SIFT_BLUR_TW* SIFT_BLUR_ROWS_PER_PASS) k_sift_blur_cols(const float* __restrict__ in, float* __restrict__ out, int w, int h,
                                                                                         SiftTaps taps) {
    __shared__ float s_t[SIFT_BLUR_TH + 2 * SIFT_MAX_RADIUS][SIFT_BLUR_TW];
    const int tx = threadIdx.x % SIFT_BLUR_TW, ty = threadIdx.x / SIFT_BLUR_TW, r = taps.radius;
    const int j = blockIdx.y * SIFT_BLUR_TW + tx, i0 = blockIdx.x * SIFT_BLUR_TH;  // rows on x: the grid's y holds 65535 at most
    const int jc = j < w ? j : w - 1;
    for (int rr = ty; rr < SIFT_BLUR_TH + 2 * r; rr += SIFT_BLUR_ROWS_PER_PASS) s_t[rr][tx] = in[(size_t)sift_mirror(i0 - r + rr, h) * w + jc];
    __syncthreads();
    for (int q = ty; q < SIFT_BLUR_TH; q += SIFT_BLUR_ROWS_PER_PASS) {
        const int i = i0 + q;
        if (i >= h || j >= w) continue;
        float sum = __fmul_rn(taps.ker[0], s_t[q + r][tx]);
        for (int k = 1; k <= r; ++k) sum = __fadd_rn(sum, __fmul_rn(taps.ker[k], __fadd_rn(s_t[q + r - k][tx], s_t[q + r + k][tx])));
        out[(size_t)i * w + j] = sum;
    }
}

// horizontal pass: SIFT_BLUR_LINE samples of one row, halo of `radius` samples left and right
__global__ void __launch_bounds__(SIFT_BLUR_LINE) k_sift_blur_rows(const float* __restrict__ in, float* __restrict__ out, int w, int h, SiftTaps taps) {
    __shared__ float s_l[SIFT_BLUR_LINE + 2 * SIFT_MAX_RADIUS];
    const int r = taps.radius, i = blockIdx.x, j0 = blockIdx.y * SIFT_BLUR_LINE, t = threadIdx.x;
    const float* row = in + (size_t)i * w;
    for (int q = t; q < SIFT_BLUR_LINE + 2 * r; q += SIFT_BLUR_LINE) s_l[q] = row[sift_mirror(j0 - r + q, w)];
    __syncthreads();
    const int j = j0 + t;
    if (j >= w) return;
    float sum = __fmul_rn(taps.ker[0], s_l[t + r]);
    for (int k = 1; k <= r; ++k) sum = __fadd_rn(sum, __fmul_rn(taps.ker[k], __fadd_rn(s_l[t + r - k], s_l[t + r + k])));
    out[(size_t)i * w + j] = sum;
}

__global__ void __launch_bounds__(256) k_sift_subsample(const float* __restrict__ in, int wi, float* __restrict__ out, int wo, int ho) {
    const long long n = (long long)wo * ho, t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const int i = (int)(t / wo), j = (int)(t % wo);
    out[t] = in[(size_t)(2 * i) * wi + 2 * j];
}

// ------------------------------------------------------------------------------------------------ discrete extrema
// DoG plane s of an octave at (i, j): plane s + 1 minus plane s of the Gaussians
__device__ inline float sift_dog(const float* __restrict__ base, size_t plane, int w, int s, int i, int j) {
    const size_t at = (size_t)i * w + j;
    return __fsub_rn(base[(size_t)(s + 1) * plane + at], base[(size_t)s * plane + at]);
}

// grid: x over the interior samples of one plane, y over the searched scales 1 .. n_planes - 3.  `count` counts every candidate;
// keys past `cap` are dropped and the launcher runs again with room for all
__global__ void __launch_bounds__(256) k_sift_extrema(const float* __restrict__ base, int w, int h, int o, float thr08, unsigned long long* __restrict__ keys,
                                                       unsigned cap, unsigned* __restrict__ count) {
    const int wi = w - 2, hi = h - 2;
    const long long n = (long long)wi * hi, t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const int i = 1 + (int)(t / wi), j = 1 + (int)(t % wi), s = 1 + (int)blockIdx.y;
    const size_t plane = (size_t)w * h;
    const float v = sift_dog(base, plane, w, s, i, j);
    if (!(fabsf(v) > thr08)) return;
    bool is_min = true, is_max = true;
    for (int ds = -1; ds <= 1; ++ds)
        for (int di = -1; di <= 1; ++di)
            for (int dj = -1; dj <= 1; ++dj) {
                if (ds == 0 && di == 0 && dj == 0) continue;
                const float u = sift_dog(base, plane, w, s + ds, i + di, j + dj);
                is_min = is_min && u > v;
                is_max = is_max && u < v;
            }
    if (!(is_min || is_max)) return;
    const unsigned slot = atomicAdd(count, 1u);
    if (slot < cap) keys[slot] = sift_key(o, s, i, j);
}

// ------------------------------------------------------------------------------------------------ refinement
// counts: [0] survivors of the interpolation, [1] survivors of the border test
__global__ void __launch_bounds__(256) k_sift_refine(SiftPlanes P, const unsigned long long* __restrict__ keys, int n, SiftKey* __restrict__ out,
                                                      unsigned* __restrict__ counts) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const unsigned long long key = keys[t];
    const int o = (int)(key >> 59), s0 = (int)((key >> 54) & 31u), i0 = (int)((key >> 27) & 0x7ffffffu), j0 = (int)(key & 0x7ffffffu);
    const int w = P.w[o], h = P.h[o], ns = P.n_planes - 1;  // DoG planes
    const float* base = P.base[o];
    const size_t plane = (size_t)w * h;
    const float delta = P.delta[o];
    SiftKey K;
    K.o = o; K.s = s0; K.alive = 0; K.x = K.y = K.sigma = 0.0f;
    int ic = i0, jc = j0, sc = s0;
    float offX = 0.0f, offY = 0.0f, offS = 0.0f, val = 0.0f;
    bool conv = false;
#define D(ss, ii, jj) sift_dog(base, plane, w, (ss), (ii), (jj))
    for (int it = 0; it < SIFT_MAX_ITER; ++it) {
        if (0 < ic && ic < h - 1 && 0 < jc && jc < w - 1) {
            const float c = D(sc, ic, jc);
            const float hXX = D(sc, ic - 1, jc) + D(sc, ic + 1, jc) - 2 * c;
            const float hYY = D(sc, ic, jc + 1) + D(sc, ic, jc - 1) - 2 * c;
            const float hSS = D(sc - 1, ic, jc) + D(sc + 1, ic, jc) - 2 * c;
            const float hXY = 0.25f * ((D(sc, ic + 1, jc + 1) - D(sc, ic + 1, jc - 1)) - (D(sc, ic - 1, jc + 1) - D(sc, ic - 1, jc - 1)));
            const float hXS = 0.25f * ((D(sc + 1, ic + 1, jc) - D(sc + 1, ic - 1, jc)) - (D(sc - 1, ic + 1, jc) - D(sc - 1, ic - 1, jc)));
            const float hYS = 0.25f * ((D(sc + 1, ic, jc + 1) - D(sc + 1, ic, jc - 1)) - (D(sc - 1, ic, jc + 1) - D(sc - 1, ic, jc - 1)));
            const float gX = 0.5f * (D(sc, ic + 1, jc) - D(sc, ic - 1, jc));
            const float gY = 0.5f * (D(sc, ic, jc + 1) - D(sc, ic, jc - 1));
            const float gS = 0.5f * (D(sc + 1, ic, jc) - D(sc - 1, ic, jc));
            const float det = hXX * hYY * hSS - hXX * hYS * hYS - hXY * hXY * hSS + 2 * hXY * hXS * hYS - hXS * hXS * hYY;
            const float aa = (hYY * hSS - hYS * hYS) / det, ab = (hXS * hYS - hXY * hSS) / det, ac = (hXY * hYS - hXS * hYY) / det;
            const float bb = (hXX * hSS - hXS * hXS) / det, bc = (hXY * hXS - hXX * hYS) / det, cc = (hXX * hYY - hXY * hXY) / det;
            offX = -aa * gX - ab * gY - ac * gS;
            offY = -ab * gX - bb * gY - bc * gS;
            offS = -ac * gX - bc * gY - cc * gS;
            val = c + 0.5f * (gX * offX + gY * offY + gS * offS);
        } else {
            offX = offY = offS = 5.0f;
        }
        if (fabsf(offX) < SIFT_OFF_MAX && fabsf(offY) < SIFT_OFF_MAX && fabsf(offS) < SIFT_OFF_MAX) {
            conv = true;
            break;
        }
        if (offX > +SIFT_OFF_MAX && ic + 1 < h - 1) ++ic;
        if (offY > +SIFT_OFF_MAX && jc + 1 < w - 1) ++jc;
        if (offX < -SIFT_OFF_MAX && ic - 1 > 0) --ic;
        if (offY < -SIFT_OFF_MAX && jc - 1 > 0) --jc;
        if (offS > +SIFT_OFF_MAX && sc + 1 < ns - 1) ++sc;
        if (offS < -SIFT_OFF_MAX && sc - 1 > 0) --sc;
    }
    if (conv) {
        atomicAdd(&counts[0], 1u);
        const float x = (ic + offX) * delta, y = (jc + offY) * delta;
        const float sigma = P.sigma[o][sc] * powf(P.sigma_ratio, offS);
        bool keep = fabsf(val) > P.thr;
        if (keep) {
            const float c = D(sc, ic, jc);
            const float hXX = D(sc, ic - 1, jc) + D(sc, ic + 1, jc) - 2 * c;
            const float hYY = D(sc, ic, jc + 1) + D(sc, ic, jc - 1) - 2 * c;
            const float hXY = ((D(sc, ic + 1, jc + 1) - D(sc, ic + 1, jc - 1)) - (D(sc, ic - 1, jc + 1) - D(sc, ic - 1, jc - 1))) / 4.0f;
            const float edge = (hXX + hYY) * (hXX + hYY) / (hXX * hYY - hXY * hXY);
            keep = !(fabsf(edge) > (SIFT_EDGE + 1) * (SIFT_EDGE + 1) / SIFT_EDGE);
        }
        if (keep) keep = !(x <= sigma || x + sigma >= (float)P.img_h || y <= sigma || y + sigma >= (float)P.img_w);
        if (keep) {
            atomicAdd(&counts[1], 1u);
            K.x = x; K.y = y; K.sigma = sigma; K.s = sc; K.alive = 1;
        }
    }
#undef D
    out[t] = K;
}

// ------------------------------------------------------------------------------------------------ gradients, where they are read
// centred differences inside, one-sided (not halved) on the border (ref:LibImages.cpp:660-740); gx along the rows' index
__device__ inline void sift_grad(const float* __restrict__ g, int w, int h, int i, int j, float& gx, float& gy) {
    const float* r = g + (size_t)i * w;
    if (j == 0) gy = r[1] - r[0];
    else if (j == w - 1) gy = r[w - 1] - r[w - 2];
    else gy = (r[j + 1] - r[j - 1]) * 0.5f;
    if (i == 0) gx = g[(size_t)w + j] - g[j];
    else if (i == h - 1) gx = g[(size_t)(h - 1) * w + j] - g[(size_t)(h - 2) * w + j];
    else gx = (g[(size_t)(i + 1) * w + j] - g[(size_t)(i - 1) * w + j]) * 0.5f;
}

__device__ inline float sift_mod2pi(float z) {
    const float y = SIFT_2PI;
    if (z < 0) {
        const int n = (int)((-z) / y) + 1;
        z += n * y;
    }
    const int n = (int)(z / y);
    return z - n * y;
}

__device__ inline void sift_fx_add(unsigned long long* bin, float v, double scale) {
    const long long q = __double2ll_rn((double)v * scale);
    if (q) atomicAdd(bin, (unsigned long long)q);
}

// ------------------------------------------------------------------------------------------------ orientations
// one wave per candidate; n_ori[c] orientations of candidate c, ascending by bin, in theta[c * SIFT_MAX_ORI ...]
__global__ void __launch_bounds__(64) k_sift_orient(SiftPlanes P, const SiftKey* __restrict__ keys, int n, const double* __restrict__ fx_scale,
                                                     int* __restrict__ n_ori, float* __restrict__ theta) {
    __shared__ unsigned long long s_acc[SIFT_ORI_BINS];
    __shared__ float s_h[2][SIFT_ORI_BINS];
    const int c = blockIdx.x, lane = threadIdx.x;
    if (c >= n) return;
    const SiftKey K = keys[c];
    if (!K.alive) {
        if (lane == 0) n_ori[c] = 0;
        return;
    }
    const int w = P.w[K.o], h = P.h[K.o];
    const float* g = P.base[K.o] + (size_t)K.s * w * h;
    const float delta = P.delta[K.o], xk = K.x / delta, yk = K.y / delta, sk = K.sigma / delta;
    const double scale = fx_scale[0];
    if (lane < SIFT_ORI_BINS) s_acc[lane] = 0ull;
    __syncthreads();
    const float R = 3 * SIFT_LAMBDA_ORI * sk;
    const int siMin = max(0, (int)((double)(xk - R) + 0.5)), sjMin = max(0, (int)((double)(yk - R) + 0.5));
    const int siMax = min((int)((double)(xk + R) + 0.5), h - 1), sjMax = min((int)((double)(yk + R) + 0.5), w - 1);
    const int nj = sjMax - sjMin + 1, ni = siMax - siMin + 1;
    const float norm = 1.0f / (2.0f * SIFT_LAMBDA_ORI * SIFT_LAMBDA_ORI);
    if (nj > 0 && ni > 0) {
        for (int q = lane; q < ni * nj; q += 64) {
            const int si = siMin + q / nj, sj = sjMin + q % nj;
            const float sX = ((float)si - xk) / sk, sY = ((float)sj - yk) / sk;
            float dx, dy;
            sift_grad(g, w, h, si, sj, dx, dy);
            const float ori = sift_mod2pi(atan2f(dy, dx));
            const float m = sqrtf(dx * dx + dy * dy) * expf(-(sX * sX + sY * sY) * norm);
            const float fb = truncf(ori / SIFT_2PI * (float)SIFT_ORI_BINS + 0.5f);
            const int bin = (int)fb % SIFT_ORI_BINS;
            if (bin >= 0 && bin < SIFT_ORI_BINS && m == m) sift_fx_add(&s_acc[bin], m, scale);
        }
    }
    __syncthreads();
    if (lane < SIFT_ORI_BINS) s_h[0][lane] = (float)((double)(long long)s_acc[lane] / scale);
    __syncthreads();
    int cur = 0;
    for (int it = 0; it < 6; ++it) {  // six box filters of three bins, circular
        if (lane < SIFT_ORI_BINS) {
            const float a = s_h[cur][(lane + SIFT_ORI_BINS - 1) % SIFT_ORI_BINS], b = s_h[cur][lane], d = s_h[cur][(lane + 1) % SIFT_ORI_BINS];
            s_h[cur ^ 1][lane] = __fadd_rn(__fadd_rn(a, b), d) / 3.0f;
        }
        __syncthreads();
        cur ^= 1;
    }
    if (lane == 0) {
        const float* H = s_h[cur];
        float mx = H[0];
        for (int b = 1; b < SIFT_ORI_BINS; ++b) mx = fmaxf(mx, H[b]);
        int k = 0;
        for (int b = 0; b < SIFT_ORI_BINS; ++b) {
            const float hc = H[b], hp = H[(b + SIFT_ORI_BINS - 1) % SIFT_ORI_BINS], hn = H[(b + 1) % SIFT_ORI_BINS];
            if (hc > SIFT_T * mx && hc > hp && hc > hn && k < SIFT_MAX_ORI) {
                const float di = (hp - hn) / (2 * (hp + hn - 2 * hc));
                const float ori = (float)(((double)((float)b + di) + 0.5) * 2 * M_PI / (double)(float)SIFT_ORI_BINS);
                theta[(size_t)c * SIFT_MAX_ORI + k++] = (double)ori > M_PI ? (float)((double)ori - 2 * M_PI) : ori;
            }
        }
        n_ori[c] = k;
    }
}

// ------------------------------------------------------------------------------------------------ descriptors
// one wave per candidate, once per orientation; rows row_ofs[c] ... of `out` (col, row, sigma, theta, 128 integers)
__global__ void __launch_bounds__(64) k_sift_describe(SiftPlanes P, const SiftKey* __restrict__ keys, int n, const double* __restrict__ fx_scale,
                                                       const int* __restrict__ n_ori, const int* __restrict__ row_ofs, const float* __restrict__ theta,
                                                       float* __restrict__ out) {
    __shared__ unsigned long long s_acc[SIFT_DESC];
    __shared__ float s_d[SIFT_DESC];
    __shared__ float s_norm;
    const int c = blockIdx.x, lane = threadIdx.x;
    if (c >= n) return;
    const int n_th = n_ori[c];
    if (n_th <= 0) return;
    const SiftKey K = keys[c];
    const int w = P.w[K.o], h = P.h[K.o];
    const float* g = P.base[K.o] + (size_t)K.s * w * h;
    const float delta = P.delta[K.o], xk = K.x / delta, yk = K.y / delta, sk = K.sigma / delta;
    const double scale = fx_scale[0];
    const float lam = SIFT_LAMBDA_DES;
    const float t2 = 1.0f / (2.0f * (lam * sk) * (lam * sk));
    const float norm1 = 1.0f / (2 * lam * sk / SIFT_NHIST), norm2 = (float)(SIFT_NORI / (2 * M_PI)), half = (SIFT_NHIST - 1.0f) / 2.0f;
    const float R = (1 + 1 / (float)SIFT_NHIST) * lam * sk;
    const float Rp = (float)(M_SQRT2 * (double)R);
    // the reference's loops stop one short of siMax / sjMax here (ref:KeyPoint.cpp:246-250)
    const int siMin = max(0, (int)((double)(xk - Rp) + 0.5)), sjMin = max(0, (int)((double)(yk - Rp) + 0.5));
    const int siMax = min((int)((double)(xk + Rp) + 0.5), h - 1), sjMax = min((int)((double)(yk + Rp) + 0.5), w - 1);
    const int ni = siMax - siMin, nj = sjMax - sjMin;
    for (int k = 0; k < n_th; ++k) {
        const float th = theta[(size_t)c * SIFT_MAX_ORI + k];
        const float cosT = cosf(-th), sinT = sinf(-th);
        for (int q = lane; q < SIFT_DESC; q += 64) s_acc[q] = 0ull;
        __syncthreads();
        if (ni > 0 && nj > 0) {
            for (int q = lane; q < ni * nj; q += 64) {
                const int si = siMin + q / nj, sj = sjMin + q % nj;
                const float X = cosT * ((float)si - xk) - sinT * ((float)sj - yk), Y = sinT * ((float)si - xk) + cosT * ((float)sj - yk);
                if (!(fabsf(X) < R && fabsf(Y) < R)) continue;
                float dx, dy;
                sift_grad(g, w, h, si, sj, dx, dy);
                const float ori = sift_mod2pi(atan2f(dy, dx) - th);
                const float M = sqrtf(dx * dx + dy * dy) * expf(-(X * X + Y * Y) * t2);
                if (!(M == M)) continue;
                const float alpha = X * norm1 + half, beta = Y * norm1 + half, gamma = ori * norm2;
                const float fi = floorf(alpha), fj = floorf(beta), fg = floorf(gamma);
                const int i0 = (int)fi, j0 = (int)fj;
                const float v0 = i0 < 0 ? 0.0f : 1.0f - fabsf(fi - alpha), v1 = i0 > SIFT_NHIST - 2 ? 0.0f : 1.0f - fabsf(fi + 1.0f - alpha);
                const float v2 = j0 < 0 ? 0.0f : 1.0f - fabsf(fj - beta), v3 = j0 > SIFT_NHIST - 2 ? 0.0f : 1.0f - fabsf(fj + 1.0f - beta);
                const float gl = 1.0f - (gamma - fg), gr = 1.0f - (fg + 1 - gamma);
                const int ia = min(max(0, i0), SIFT_NHIST - 1), ib = min(ia + 1, SIFT_NHIST - 1);
                const int ja = min(max(0, j0), SIFT_NHIST - 1), jb = min(ja + 1, SIFT_NHIST - 1);
                const int gi = (int)gamma;
                const int bl = ((gi % SIFT_NORI) + SIFT_NORI) % SIFT_NORI, br = (((gi + 1) % SIFT_NORI) + SIFT_NORI) % SIFT_NORI;
                sift_fx_add(&s_acc[(ia * SIFT_NHIST + ja) * SIFT_NORI + bl], gl * v0 * v2 * M, scale);
                sift_fx_add(&s_acc[(ia * SIFT_NHIST + ja) * SIFT_NORI + br], gr * v0 * v2 * M, scale);
                sift_fx_add(&s_acc[(ia * SIFT_NHIST + jb) * SIFT_NORI + bl], gl * v0 * v3 * M, scale);
                sift_fx_add(&s_acc[(ia * SIFT_NHIST + jb) * SIFT_NORI + br], gr * v0 * v3 * M, scale);
                sift_fx_add(&s_acc[(ib * SIFT_NHIST + ja) * SIFT_NORI + bl], gl * v1 * v2 * M, scale);
                sift_fx_add(&s_acc[(ib * SIFT_NHIST + ja) * SIFT_NORI + br], gr * v1 * v2 * M, scale);
                sift_fx_add(&s_acc[(ib * SIFT_NHIST + jb) * SIFT_NORI + bl], gl * v1 * v3 * M, scale);
                sift_fx_add(&s_acc[(ib * SIFT_NHIST + jb) * SIFT_NORI + br], gr * v1 * v3 * M, scale);
            }
        }
        __syncthreads();
        for (int q = lane; q < SIFT_DESC; q += 64) s_d[q] = (float)((double)(long long)s_acc[q] / scale);
        __syncthreads();
        if (lane == 0) {  // the reference's serial sums, in its order
            float l2 = 0.0f;
            for (int q = 0; q < SIFT_DESC; ++q) l2 = __fadd_rn(l2, __fmul_rn(s_d[q], s_d[q]));
            s_norm = sqrtf(l2) * 0.2f;
        }
        __syncthreads();
        const float thresh = s_norm;
        for (int q = lane; q < SIFT_DESC; q += 64) s_d[q] = fminf(s_d[q], thresh);
        __syncthreads();
        if (lane == 0) {
            float l2 = 0.0f;
            for (int q = 0; q < SIFT_DESC; ++q) l2 = __fadd_rn(l2, __fmul_rn(s_d[q], s_d[q]));
            s_norm = 512.0f / sqrtf(l2);
        }
        __syncthreads();
        const float tQ = s_norm;
        float* row = out + (size_t)(row_ofs[c] + k) * SIFT_ROW;
        if (lane == 0) {
            row[0] = K.y; row[1] = K.x; row[2] = K.sigma; row[3] = th;
        }
        for (int q = lane; q < SIFT_DESC; q += 64) {
            const float v = s_d[q] * tQ;
            row[4 + q] = v == v ? (float)min((int)v, 255) : 0.0f;
        }
        __syncthreads();
    }
}
