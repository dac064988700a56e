// satba_diag_split.h -- where the unit-weight front beside the factorisation cuts its diagonal pass in two (satba_schur_api.inc:
// SchurRoute::c_split).  Plain C++, no HIP: a host program can check the rule without a device (tests/host/diag_split_dump.cpp).
#pragma once

namespace satba {
// The reduced system has M cameras x NP unknowns, in T = ceil(M NP / 64) tile columns of 64; the factorisation beside the pair kernel
// (satba_chol3.h) reaches tile column k at its step k, the last ones long after the pair kernel has ended.  The diagonal blocks and
// right-hand-side entries of the cameras in the last `late_cols` tile columns are therefore produced BEHIND the pair kernel, camera by
// camera, instead of in front of it.
// Returns c*, the first late camera: cameras [0, c*) stay in front, cameras [c*, M) go behind.
//   c* = the first camera with a column in tile column T - late_cols (or beyond), i.e. with a column >= b = 64 (T - late_cols):
//   camera c owns columns c NP .. c NP + NP - 1, so c* = floor(b / NP).  A camera that STRADDLES the boundary b is late (the tile
//   column that needs it is a late one); every camera < c* has all its columns in front of b.
//   late_cols <= 0: M (nothing late); late_cols >= T: 0 (everything late).
// applies: the route takes a split at all (one rank, unit weights, factorisation beside the pair kernel); otherwise M.
inline int diag_split_tiles(int M, int NP) { return (M * NP + 63) / 64; }
inline int diag_split_camera(int M, int NP, int late_cols, bool applies = true) {
    if (!applies || late_cols <= 0 || M <= 0 || NP <= 0) return M;
    const int T = diag_split_tiles(M, NP);
    if (late_cols >= T) return 0;
    const int c = 64 * (T - late_cols) / NP;
    return c < M ? c : M;
}
// SATBA_DIAG_LATE_FROM=<camera> (tests): c* directly, anywhere in [0, M]
inline int diag_split_forced(int M, int from, bool applies = true) {
    if (!applies) return M;
    return from < 0 ? 0 : (from > M ? M : from);
}
// Tile columns that go late by default: 3 of 16, the best of the sweep at 200 cameras x 5 (profiles/diag_late_ab.txt:
// cameras 166 .. 199 late; one column more and the chain waits a step longer for the late part, one column fewer and the part in front
// no longer fits one dispatch round).  It scales with T -- 3 T / 16, rounded down -- because what it rests on does: the chain is a fixed
// SHARE of its steps behind the pair kernel's end (5 of 16 there), whatever T is.  Only T = 16 has been measured.
inline int diag_late_cols_default(int T) { return 3 * T / 16; }
// ... and where the late part runs: false (a) a launch of its own behind the pair kernel | true (b) the trailing workgroups of the pair launch
constexpr bool DIAG_LATE_TAIL_DEFAULT = true;
}  // namespace satba
