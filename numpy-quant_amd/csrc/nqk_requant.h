// The arithmetic that nqk_quant.hip's elementwise kernels and nqk_gemm16.hip's fused epilogue share:
// the quantize bounds, NumPy's float -> int64 conversion, the zero-point term of a q_matmul output
// and the quantize half of requantize.  Every function restates NumPy 2.2 bit for bit (the rules
// are at the head of nqk_quant.hip); a file that includes this is built -ffp-contract=off with the
// correctly rounded f32 divide.
#pragma once
#include "nqk_common.h"

namespace nqk {

__device__ __forceinline__ int64_t f64_to_i64(double u) {
  // NaN / +-inf / |u| >= 2^63 -> INT64_MIN (x86 integer-indefinite), else exact.
  if (!(u > -9223372036854775808.0 && u < 9223372036854775808.0)) {
    if (u == -9223372036854775808.0) return INT64_MIN;
    return INT64_MIN;
  }
  return (int64_t)u;
}

struct QuantP {
  float scale;
  double zp;     // f64(zero point)
  int has_zp;
  double lo, hi; // Python-float bounds (f64 exact for bw <= 53)
  float flo, fhi;
};

inline QuantP make_qp(float scale, int64_t zp, int has_zp, int bw) {
  QuantP p;
  p.scale = scale;
  p.zp = (double)zp;
  p.has_zp = has_zp;
  p.lo = -__builtin_ldexp(1.0, bw - 1);
  p.hi = __builtin_ldexp(1.0, bw - 1) - 1.0;
  p.flo = (float)p.lo;
  p.fhi = (float)p.hi;
  return p;
}

struct ZpT {
  int flags;
  int64_t zp, zpa, zpb, K, M, N;
  const int64_t* row;
  const int64_t* col;
  BatchMap bm;
};

inline ZpT make_zp(int flags, int64_t zp, int64_t zpa, int64_t zpb, int64_t K, int64_t M, int64_t N,
                   const int64_t* row, const int64_t* col, const int64_t* bmap) {
  ZpT z;
  z.flags = flags; z.zp = zp; z.zpa = zpa; z.zpb = zpb; z.K = K; z.M = M; z.N = N;
  z.row = row; z.col = col; z.bm = batch_map(bmap);
  return z;
}

__device__ __forceinline__ int64_t zp_term(const ZpT& z, int64_t b, int64_t m, int64_t n) {
  int64_t t = 0;
  if (z.flags & NQK_ZP_FULL) t += z.row[(b * z.M + m) * z.N + n];
  if (z.flags & NQK_ZP_SCALAR) t += z.zp;
  if (z.flags & NQK_ZP_ROW) t += z.row[map_a(z.bm, b) * z.M + m] * z.zpb;
  if (z.flags & NQK_ZP_COL) t += z.col[map_b(z.bm, b) * z.N + n] * z.zpa;
  if (z.flags & NQK_ZP_KCONST) t -= z.zpa * z.zpb * z.K;
  return t;
}

// the quantize half of requantize (numpy_quantization.py:69-72) of one dequantized value d:
// vv = f32(r * d), then rint and clip in f64 with a result zero point, in f32 without
__device__ __forceinline__ int64_t requant_tail(float d, float r, double rz, int has_rz, double lo, double hi,
                                                float flo, float fhi) {
  float vv = r * d;
  int64_t o;
  if (has_rz) {
    double u = __builtin_rint(rz + (double)vv);
    if (u != u) o = INT64_MIN;
    else { u = u < lo ? lo : u; u = u > hi ? hi : u; o = f64_to_i64(u); }
  } else {
    float u = __builtin_rintf(vv);
    if (u != u) o = INT64_MIN;
    else { u = u < flo ? flo : u; u = u > fhi ? fhi : u; o = f64_to_i64((double)u); }
  }
  return o;
}

}  // namespace nqk
