// XCD-aware tile orders (part of nqk_common.h; plain C++ so that a host-only program can
// check the arithmetic, tests/test_xcd_remap.py).
//
// The hardware deals workgroups round-robin over the device's XC XCDs (workgroup b runs on
// XCD b % XC, MI355X_MICROARCH.md).  The tile ids 0 .. T-1 are row-panel major; they are cut
// into XC contiguous bands, band x served by the workgroups of XCD x, so that tiles which
// share operand rows share an L2.  Every map below must be a permutation of 0 .. T-1 for
// ANY XC >= 1 (the XCD count is a device attribute, or NQK_XCDS), not only for 8.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NQK_HD __host__ __device__
#else
#define NQK_HD
#endif

namespace nqk {

// One tile per workgroup (k_embed_q, k_embed_q16, k_qgemm_big): workgroup b of T
// takes tile xcd_remap(b, T, XC).  Band x holds T / XC tiles, one more in the first T % XC
// bands — exactly the number of workgroups b < T with b % XC == x, whose b / XC counts them.
template <typename I>
NQK_HD constexpr I xcd_remap(I b, I T, I XC) {
  const I x = b % XC, q = T / XC, r = T % XC;
  return x * q + (x < r ? x : r) + b / XC;
}

// Persistent workgroups (k_pg): workgroup b of G walks `iters` tiles first, first + step, ...
// of the T tiles; the workgroups with b % X == x (X = min(G, XC)) share the band
// [T x / X, T (x + 1) / X) and stride over it by their count.
struct XcdWalk {
  int first, step, iters;
};
NQK_HD constexpr XcdWalk xcd_walk(int b, int G, int T, int XC) {
  const int X = G < XC ? G : XC, x = b % X;
  const int nx = (G - x + X - 1) / X;
  const int lo = (int)((int64_t)T * x / X), hi = (int)((int64_t)T * (x + 1) / X);
  const int first = lo + b / X;
  return XcdWalk{first, nx, first < hi ? (hi - first + nx - 1) / nx : 0};
}

}  // namespace nqk
