// The cells of the windowed matcher (include/satba.h, satba_match_window): per pair a grid over the selected
// keypoints of the second image, the cell of a coordinate, and the cells a query has to visit.  Plain C++17 in float64 that compiles
// on the host on its own (tests/host/window_cells_dump.cpp); the kernels of satba_window.h run the same functions.
//
// Why a query's range covers its candidates.  A candidate j of a query at e has fabs(fl(e - e_j)) < r.  Rounding is monotone and r
// is a double, so the exact |e - e_j| is below r too: e - r < e_j < e + r in real numbers.  fl(e - r) may lie above e - r, by at
// most half a unit in its last place; one step of nextafter below it lies at or below e - r, hence below e_j.  (The step is a
// margin, not a need: fl(e - r) is a double next to e - r, no double lies strictly between the two, and e_j is a double above
// e - r, so e_j >= fl(e - r) already.  It costs one cell more in the rare query whose bound sits on a cell's edge.)  wc_cell is monotone
// non-decreasing in the coordinate -- a rounded subtraction of a constant, a rounded division by a positive constant, floor and a
// clamp are each monotone -- so wc_cell(lo) <= wc_cell(e_j), and in the same way wc_cell(e_j) <= wc_cell(hi).  Nothing else is used:
// the range may hold a cell too many, never one too few, whatever the cell size, the clamp or the cap do.
//
// The cap.  An axis has at most WC_MAX_DIM cells; where the extent asks for more, the cells are widened (never narrowed: the edge
// stays >= r, so a query visits at most four cells per axis, three but for rounding).  No table per cell exists anywhere: the cells
// only order a sort (satba_window.h), so a sparse grid costs nothing.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define WC_HD __host__ __device__ inline
#else
#define WC_HD inline
#endif

constexpr int WC_DIM_BITS = 20;
constexpr int WC_MAX_DIM = 1 << WC_DIM_BITS;  // cells per axis
constexpr int WC_PAIR_BITS = 64 - 2 * WC_DIM_BITS;

struct WcAxis {
    double o, w;  // origin (the smallest coordinate), cell edge (>= r; +inf with one cell)
    int n;        // cells, 1 .. WC_MAX_DIM
};
struct WcGrid { WcAxis x, y; };

// the axis over coordinates lo .. hi (lo > hi: no keypoint) for a window half-width r > 0 (may be +inf)
WC_HD WcAxis wc_axis(double lo, double hi, double r) {
    WcAxis a;
    a.o = lo; a.w = r; a.n = 1;
    const double ext = hi - lo;
    if (!(ext > 0.0) || !std::isfinite(ext) || !std::isfinite(r)) {
        if (!std::isfinite(lo)) a.o = 0.0;
        return a;
    }
    const double cells = ext / r;
    if (cells >= (double)(WC_MAX_DIM - 1)) {
        a.w = ext / (double)(WC_MAX_DIM - 1);  // >= r
        if (a.w < r) a.w = r;
        a.n = WC_MAX_DIM;
    } else {
        a.n = (int)std::floor(cells) + 1;
    }
    return a;
}

// the cell of coordinate v, 0 .. n - 1: monotone non-decreasing in v; -inf, +inf and values outside the extent are clamped
WC_HD int wc_cell(const WcAxis& a, double v) {
    if (a.n == 1) return 0;
    const double t = std::floor((v - a.o) / a.w);
    if (!(t > 0.0)) return 0;
    if (t >= (double)(a.n - 1)) return a.n - 1;
    return (int)t;
}

// the cells c0 .. c1 that hold every candidate of a query at v (see the head of the file)
WC_HD void wc_range(const WcAxis& a, double v, double r, int& c0, int& c1) {
    const double lo = nextafter(v - r, -INFINITY), hi = nextafter(v + r, INFINITY);
    c0 = wc_cell(a, lo);
    c1 = wc_cell(a, hi);
}

// sort key of a second-side keypoint: (pair, cell_y, cell_x); the cells of one grid row are consecutive
WC_HD uint64_t wc_key(int pair, int cy, int cx) {
    return ((uint64_t)(uint32_t)pair << (2 * WC_DIM_BITS)) | ((uint64_t)(uint32_t)cy << WC_DIM_BITS) | (uint64_t)(uint32_t)cx;
}
