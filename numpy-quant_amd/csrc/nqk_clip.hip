// Weight clipping search (opt-in: Model.quantize(weight_clip="mse"); not the reference's behaviour):
// for every column n of w [rows][ld] and every candidate g < G the squared error of quantizing the
// column with the shrunk scale s = f32(s0[n] * ratio[g]), and the first candidate with the smallest.
//
//   s         = f32(s0[n] * ratio[g])                        one f32 multiply
//   q         = rint(clip(f32(w[k][n] / s), f32(lo), f32(hi)))      nqk_quantize_cols' integers
//   dq        = f32(f64(q) * f64(s))                         nqk_dequantize_cols' value
//   d         = f64(w[k][n]) - f64(dq)
//   err[g][n] = sum_k RN64(d * d)                            f64, never contracted into an fma
//   index[n]  = the first g with the smallest err[g][n]:  best = err[0][n]; a later g replaces it
//               only when err[g][n] < best (a NaN never does, so a column of NaN errors gives 0)
//   scale[n]  = f32(s0[n] * ratio[index[n]])
// lo = -2^(bw-1), hi = 2^(bw-1) - 1, 1 <= bw <= 8.  |q| <= 128 has 8 significant bits and s 24, so
// f64(q) * f64(s) is exact and its rounding to f32 is the f32 product q * s: the kernel multiplies
// in f32.  The divide is the IEEE f32 divide of nqk_quantize_cols, never a reciprocal multiply.
//
// The order of the f64 sum of a column, whatever the shape of the call:
//   partial j (j = 0..63) adds the terms of rows k = j, j + 64, j + 128, .. in increasing k to +0.0;
//   then six butterfly steps m = 32, 16, 8, 4, 2, 1: p[j] = p[j] + p[j ^ m] for all j at once.
//   After the last step all 64 entries are equal: that value is err[g][n].
// (tests/_clip_ref.py restates it in NumPy.)
//
// A column whose s0 is 0 or not finite is returned as it is: scale = s0, index = 0, err = +0.0.
//
// Work split.  One workgroup of four waves per column; lane j of every wave owns partial j, so the
// butterfly is six lane exchanges and nothing is reduced across workgroups.  The candidates are
// dealt to the waves, g = 4 i + wave (i < 16): a wave's scales are uniform over its lanes, its 16
// f64 accumulators take 32 VGPRs, and the 16 divide chains of one element are independent, which
// is all the latency hiding the VALU-bound loop needs (about 20 VALU instructions per element and
// candidate, half of them the divide).  A column per workgroup gives cols * 4 waves of equal
// length: 3072 for N = 768, three on every SIMD of 256 CUs, where any wider panel leaves a
// quarter of the device idle at that N.  The price is a strided read: a wave load touches 64
// lines, of which it uses 4 bytes each, and the other waves of the workgroup and the workgroups of
// the 31 neighbouring columns, which run at the same time, find the same lines in L1 / L2.  The
// matrix is read once from HBM; the loop issues the next round's load before it computes this one.
// The totals meet in 512 bytes of LDS, where one lane takes the first minimum.
#include "nqk_common.h"

namespace nqk {
namespace {

constexpr int kClipWaves = 4;   // waves of a workgroup
constexpr int kClipPer = 16;    // candidates of a wave: g = 4 i + wave
constexpr int kClipMaxG = kClipWaves * kClipPer;

__global__ void __launch_bounds__(64 * kClipWaves)
k_clip_search(const float* __restrict__ w, int64_t rows, int64_t cols, int64_t ld, const float* __restrict__ s0v,
              const float* __restrict__ ratio, int G, float flo, float fhi, float* __restrict__ scale,
              int32_t* __restrict__ index, double* __restrict__ err) {
  __shared__ double tot[kClipMaxG];
  const int64_t n = blockIdx.x;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const float s0 = s0v[n];
  if (s0 == 0.0f || !(__builtin_fabsf(s0) < __builtin_inff())) {  // 0, +-inf, NaN: the column stays
    if (threadIdx.x == 0) { scale[n] = s0; index[n] = 0; }
    if (err && (int)threadIdx.x < G) err[(int64_t)threadIdx.x * cols + n] = 0.0;
    return;
  }
  float s[kClipPer];
  double acc[kClipPer];
#pragma unroll
  for (int i = 0; i < kClipPer; ++i) {
    const int g = kClipWaves * i + wave;
    s[i] = g < G ? s0 * ratio[g] : 1.0f;  // a candidate past G is computed and dropped
    acc[i] = 0.0;
  }
  const float* col = w + n;
  // every load is unconditional, of a row clamped to the last one, so that the wait for this
  // round's value leaves the next round's load in flight
  const int64_t last = rows - 1;
  float raw = col[(lane < last ? lane : last) * ld];
  for (int64_t k0 = 0; k0 < rows; k0 += 64) {
    // a row past the end is 0: q = 0, d = 0, and acc + 0.0 is acc (acc >= +0 or NaN)
    const float x = k0 + lane < rows ? raw : 0.0f;
    const int64_t kn = k0 + 64 + lane;
    raw = col[(kn < last ? kn : last) * ld];
    const double xd = (double)x;
#pragma unroll
    for (int i = 0; i < kClipPer; ++i) {
      float t = x / s[i];
      t = t < flo ? flo : t;
      t = t > fhi ? fhi : t;  // a NaN passes both and stays
      const float dq = __builtin_rintf(t) * s[i];
      const double d = xd - (double)dq;
      acc[i] = acc[i] + d * d;
    }
  }
#pragma unroll
  for (int i = 0; i < kClipPer; ++i) {
    double v = acc[i];
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) v = v + __shfl_xor(v, m, 64);
    const int g = kClipWaves * i + wave;
    if (lane == 0 && g < G) tot[g] = v;
  }
  __syncthreads();
  if (err && (int)threadIdx.x < G) err[(int64_t)threadIdx.x * cols + n] = tot[threadIdx.x];
  if (threadIdx.x == 0) {
    double best = tot[0];
    int bi = 0;
    for (int g = 1; g < G; ++g) {
      const double e = tot[g];
      if (e < best) { best = e; bi = g; }
    }
    scale[n] = s0 * ratio[bi];
    index[n] = bi;
  }
}

}  // namespace
}  // namespace nqk

using namespace nqk;

extern "C" int nqk_clip_search_cols(const float* w, int64_t rows, int64_t cols, int64_t ld, const float* s0,
                                    const float* ratio, int G, int bit_width, float* scale, int32_t* index,
                                    double* err) {
  if (rows < 1 || cols < 1) return fail("nqk_clip_search_cols: empty matrix");
  if (ld < cols) return fail("nqk_clip_search_cols: ld < cols");
  if (G < 1 || G > kClipMaxG) return fail("nqk_clip_search_cols: G must be in 1..64");
  if (bit_width < 1 || bit_width > 8) return fail("nqk_clip_search_cols: bit_width must be in 1..8");
  if (!w || !s0 || !ratio || !scale || !index) return fail("nqk_clip_search_cols: null pointer");
  if ((uintptr_t)w % 4 || (uintptr_t)s0 % 4 || (uintptr_t)ratio % 4 || (uintptr_t)scale % 4 ||
      (uintptr_t)index % 4 || (uintptr_t)err % 8)
    return fail("nqk_clip_search_cols: w, s0, ratio, scale and index need 4-byte alignment, err 8-byte");
  if (cols > 0x7fffffff || rows > ((int64_t)1 << 40) || ld > ((int64_t)1 << 40))
    return fail("nqk_clip_search_cols: more than 2^31 - 1 columns or 2^40 rows");
  const float flo = -__builtin_ldexpf(1.0f, bit_width - 1), fhi = __builtin_ldexpf(1.0f, bit_width - 1) - 1.0f;
  hipLaunchKernelGGL(k_clip_search, dim3((unsigned)cols), dim3(64 * kClipWaves), 0, stream(), w, rows, cols, ld, s0,
                     ratio, G, flo, fhi, scale, index, err);
  return launch_status("nqk_clip_search_cols");
}
