// satba_elbow.h -- the elbow of an ascending curve and its success test (ref:bundle_adjust/ba_outliers.py:14-58 `get_elbow_value`
// at max_outliers_percent = 20), shared by the per-camera threshold of the outlier rejection (k_out_elbow, satba_outliers.h) and the
// per-pair threshold of the UTM filter (k_utm_threshold, satba_utm.h).  Each caller applies its own last step to (elbow, success,
// v[n - 1]).
//   elbow = v[argmax_i dist((i, v_i), chord)], success = elbow >= percentile(v, 100 - 20)
// The result must agree with numpy index for index, also where only rounding decides (get_elbow_value([1.0, 9.0]) is 9.0: the two
// distances to the chord are rounding noise), so every product and sum rounds where numpy's does:
//   * no contraction.  HIP's __dmul_rn / __dadd_rn / __dsub_rn are inline functions around the plain operators and carry the
//     translation unit's default (-ffp-contract=fast), so the compiler fused their products into the sums that follow -- k_out_elbow
//     was written with them until the plateau vectors of tests/cases_outliers.py (maxima that only rounding tells apart) and the
//     two-point camera showed another argmax than numpy's.  The operators below are written out under the pragma, which has to stand
//     in every function: it does not reach into a callee;
//   * the first maximum wins, like np.argmax; n == 1 (the chord is a point and numpy's distances are NaN) gives argmax 0;
//   * numpy 2.x's "linear" percentile with its two-sided lerp.
// The pieces are plain C++ that also compiles on the host (tests/host/utm_dump.cpp runs elbow_sequential); elbow_block is the
// workgroup's version of the same argmax.
#pragma once
#include <cmath>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ELB_HD __host__ __device__ inline
#else
#define ELB_HD inline
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#define ELB_SQRT(x) __dsqrt_rn(x)
#define ELB_DIV(a, b) __ddiv_rn(a, b)
#else
#define ELB_SQRT(x) std::sqrt(x)
#define ELB_DIV(a, b) ((a) / (b))
#endif

namespace satba {

struct ElbowChord {  // from (0, v0) to (n - 1, v_last), normalised (numpy: line_vec / sqrt(sum(line_vec ** 2)))
    double v0, ux, uy;
};
struct Elbow {
    double elbow;  // v[argmax]
    bool success;  // the curve is L-shaped: the elbow is not below the 80th percentile
    double last;   // v[n - 1]
};

ELB_HD ElbowChord elbow_chord(const double* v, int n) {
#pragma clang fp contract(off)
    const double lx = (double)(n - 1), ly = v[n - 1] - v[0];
    const double lxx = lx * lx, lyy = ly * ly;
    const double nrm = ELB_SQRT(lxx + lyy);
    return ElbowChord{v[0], ELB_DIV(lx, nrm), ELB_DIV(ly, nrm)};
}

// distance of (i, v_i) to the chord
ELB_HD double elbow_distance(const ElbowChord& c, int i, double vi) {
#pragma clang fp contract(off)
    const double px = (double)i, py = vi - c.v0;
    const double pxu = px * c.ux, pyu = py * c.uy;
    const double sp = pxu + pyu;
    const double spx = sp * c.ux, spy = sp * c.uy;
    const double qx = px - spx, qy = py - spy;
    const double qxx = qx * qx, qyy = qy * qy;
    return ELB_SQRT(qxx + qyy);
}

// from the first maximum (best, arg) of the distances to the result
ELB_HD Elbow elbow_finish(const double* v, int n, double best, int arg) {
#pragma clang fp contract(off)
    if (!(best >= 0.0) || arg >= n) arg = 0;  // n == 1: the chord is a point and numpy's distances are NaN -> argmax 0
    const double elbow = v[arg];
    // np.percentile(err, 80), linear interpolation with numpy's two-sided lerp.  Virtual index: method "linear" of numpy 2.2
    // (numpy/lib/_function_base_impl.py, _QuantileMethods["linear"]: get_virtual_index = (n - 1) * quantiles, NOT the generic
    // n q + (alpha + q (1 - alpha - beta)) - 1 of the other methods); checked bit for bit against np.percentile for n < 3000
    // in tests/test_host_logic.py
    const double vi = (double)(n - 1) * 0.8;
    const int lo = (int)floor(vi), hi = lo + 1 < n - 1 ? lo + 1 : n - 1;
    const double t = vi - (double)lo, a = v[lo], bb = v[hi], diff = bb - a;
    const double dt = diff * t;
    double pct = a + dt;
    if (t >= 0.5) {
        const double t1 = 1.0 - t;
        const double d1 = diff * t1;
        pct = bb - d1;
    }
    return Elbow{elbow, !(elbow < pct), v[n - 1]};
}

// one thread over v[0 .. n), n >= 1
ELB_HD Elbow elbow_sequential(const double* v, int n) {
    const ElbowChord c = elbow_chord(v, n);
    double best = -1.0;
    int best_i = 0x7fffffff;
    for (int i = 0; i < n; ++i) {
        const double d = elbow_distance(c, i, v[i]);
        if (d > best) { best = d; best_i = i; }
    }
    return elbow_finish(v, n, best, best_i);
}

#if defined(__HIPCC__) || defined(__CUDACC__)
// one workgroup of THREADS (a power of two) over v[0 .. n), n >= 1; every thread calls it, the result is thread 0's
template <int THREADS>
__device__ inline Elbow elbow_block(const double* __restrict__ v, int n) {
    const ElbowChord c = elbow_chord(v, n);
    double best = -1.0;
    int best_i = 0x7fffffff;
    for (int i = threadIdx.x; i < n; i += THREADS) {
        const double d = elbow_distance(c, i, v[i]);
        if (d > best) { best = d; best_i = i; }  // ascending i per thread: the first maximum of the thread's subset
    }
    __shared__ double s_d[THREADS];
    __shared__ int s_i[THREADS];
    s_d[threadIdx.x] = best; s_i[threadIdx.x] = best_i;
    __syncthreads();
    for (int s = THREADS / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            const double d2 = s_d[threadIdx.x + s];
            const int i2 = s_i[threadIdx.x + s];
            if (d2 > s_d[threadIdx.x] || (d2 == s_d[threadIdx.x] && i2 < s_i[threadIdx.x])) { s_d[threadIdx.x] = d2; s_i[threadIdx.x] = i2; }
        }
        __syncthreads();
    }
    if (threadIdx.x != 0) return Elbow{0.0, false, 0.0};
    return elbow_finish(v, n, s_d[0], s_i[0]);
}
#endif

}  // namespace satba
