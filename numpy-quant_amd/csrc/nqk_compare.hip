// Error statistics of a quantized model's value against the float model's (compare.py): one
// streaming pass over both arrays, accumulated into 8 words of state per value.
//
//   x      float32: the float model's value
//   y      float32, or the integer storage of a QTensor with its scale and a scalar (or no) zero
//          point, dequantized per element as k_dequantize and nqk_topk_softmax do and never
//          written anywhere: y = f32(f64(q - zp) * f64(scale))
//   pair   skipped when x or the float32 y is NaN or +-inf (counted in word 1, nothing else);
//          otherwise d = f64(x) - f64(y) and the terms |d|, d * d, f64(x) * f64(x)
//   state  int64 n_compared, int64 n_skipped, f64 sum|d|, f64 sum d^2, f64 sum x^2, f64 max|d|,
//          two reserved words; a fresh state is all zero bytes
//
// The three sums are float64 additions in one fixed order, the same for every grid, so a state
// is a function of the data and the call order alone.  The order (compare.host_state restates it
// in NumPy):
//   chunk   c covers elements [4096 c, 4096 (c + 1)); lane t of 256 adds the terms of elements
//           4096 c + 1024 j + 4 t + k, j = 0..3 outer, k = 0..3 inner, to +0.0 (four 16-byte
//           loads of f32 per lane, each wave reading 1 KiB at a stretch).  Absent and skipped
//           elements add +0.0, which changes nothing: every term is >= +0.
//   fold    the 256 lane sums by adjacent pairs, v = v[0::2] + v[1::2] until one is left: inside
//           a wave the xor butterfly 1, 2, .., 32 (an addition commutes, so both lanes of a pair
//           hold the same bits), then (W0 + W1) + (W2 + W3) of the four wave totals.
//   pass 1  k_cmp_chunks writes every chunk's three partials to scratch[s * chunks + c];
//           workgroups take chunks grid-stride, which moves work around and no addition.
//   pass 2  k_cmp_final, one workgroup per sum: lane t adds the partials of chunks t, t + 256, ..
//           in increasing order to +0.0, the 256 lane sums fold as above, and the total is added
//           to the state word: one float64 addition per word and call.
// The counts are integer additions and the maximum is exact in any order (non-negative doubles
// order as their bit patterns): a workgroup reduces both over all its chunks and touches the
// state with at most one atomic per word, the maximum only after reading that it would move it
// (hist_block_end's rule, nqk_hist.hip).
//
// x and y need the alignment of their elements only: a lane's four elements are read as one
// pack whose alignment is the element's, which the hardware takes in one access.  The last,
// partial chunk is read element by element under its bound.
#include <stdlib.h>
#include "nqk_common.h"

namespace nqk {
namespace {

constexpr int kCmpChunk = NQK_CMP_CHUNK;
constexpr int kCmpFinalUnroll = 32;  // partials in flight per lane in pass 2
static_assert(kCmpChunk == 4096, "256 lanes x 4 groups x 4 elements");

// four consecutive elements at the alignment of one
template <typename T>
struct __attribute__((packed, aligned(sizeof(T)))) CmpPack {
  T e[4];
};

// ZP32: q and zp both fit 31 bits (int8 / int16 storage, |zp| <= 2^30), so q - zp is exact in
// int32 and converts to float64 in one instruction; the value is the same either way.
template <typename T, bool ZP32>
__device__ __forceinline__ float cmp_cvt(T q, int64_t zp, double scale) {
  if (ZP32) return (float)((double)((int)q - (int)zp) * scale);
  return (float)((double)((int64_t)q - zp) * scale);  // k_dequantize, scalar or no zero point
}
template <>
__device__ __forceinline__ float cmp_cvt<float, false>(float y, int64_t, double) { return y; }

__device__ __forceinline__ bool cmp_finite(float v) { return (__float_as_uint(v) & 0x7F800000u) != 0x7F800000u; }

struct CmpLane {  // what one lane carries: sums of one chunk, maximum and skips of all its chunks
  double sa = 0.0, sd = 0.0, sx = 0.0, mx = 0.0;
  uint32_t skipped = 0;  // a workgroup sees fewer than 2^32 elements: cmp_grid bounds its chunks
};

// A skipped pair is taken as (+0, +0): d, |d|, d * d and x * x are then +0, which adds nothing
// to sums that start at +0 and never moves the maximum.  Two selects instead of one per term.
__device__ __forceinline__ void cmp_take(float x, float y, CmpLane& l) {
  const bool ok = cmp_finite(x) && cmp_finite(y);
  const double xd = (double)(ok ? x : 0.0f);
  const double d = xd - (double)(ok ? y : 0.0f);
  const double ad = __builtin_fabs(d);
  l.sa += ad;
  l.sd += d * d;
  l.sx += xd * xd;
  l.mx = __builtin_fmax(l.mx, ad);  // neither is a NaN
  l.skipped += ok ? 0u : 1u;
}

// v + the value of lane (lane ^ off), the same bits in both lanes of a pair.  Inside a row of 16
// lanes by DPP: the two quad exchanges, then row_half_mirror and row_mirror, which by then pair a
// lane with one that holds what its xor partner holds; across rows by ds_bpermute.  All 64 lanes
// must be active.
template <int CTRL>
__device__ __forceinline__ double cmp_dpp(double v) {
  const uint64_t b = (uint64_t)__double_as_longlong(v);
  const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)b, CTRL, 0xF, 0xF, false);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(b >> 32), CTRL, 0xF, 0xF, false);
  return __longlong_as_double((long long)(((uint64_t)hi << 32) | lo));
}
constexpr int kDppQuadXor1 = 0xB1, kDppQuadXor2 = 0x4E, kDppRowHalfMirror = 0x141, kDppRowMirror = 0x140;

__device__ __forceinline__ double cmp_wave_fold(double v) {
  v += cmp_dpp<kDppQuadXor1>(v);
  v += cmp_dpp<kDppQuadXor2>(v);
  v += cmp_dpp<kDppRowHalfMirror>(v);
  v += cmp_dpp<kDppRowMirror>(v);
  v += __shfl_xor(v, 16, 64);
  v += __shfl_xor(v, 32, 64);
  return v;
}

template <typename T, bool ZP32>
__global__ void __launch_bounds__(256)
k_cmp_chunks(const float* __restrict__ x, const T* __restrict__ y, double scale, int64_t zp, int64_t n,
             int64_t nchunks, int64_t* __restrict__ state, double* __restrict__ scratch) {
  __shared__ double part[2][3][4];
  __shared__ double wmx[4];
  __shared__ uint32_t wskip[4];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  CmpLane l;
  int par = 0;
  for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x, par ^= 1) {
    const int64_t base = c * kCmpChunk + 4 * t;
    l.sa = l.sd = l.sx = 0.0;
    if ((c + 1) * kCmpChunk <= n) {  // a whole chunk (the same answer in every lane)
      CmpPack<float> xv[4];
      CmpPack<T> yv[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        xv[j] = *reinterpret_cast<const CmpPack<float>*>(x + base + 1024 * j);
        yv[j] = *reinterpret_cast<const CmpPack<T>*>(y + base + 1024 * j);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int k = 0; k < 4; ++k) cmp_take(xv[j].e[k], cmp_cvt<T, ZP32>(yv[j].e[k], zp, scale), l);
    } else {
      for (int j = 0; j < 4; ++j)
        for (int k = 0; k < 4; ++k) {
          const int64_t i = base + 1024 * j + k;
          if (i < n) cmp_take(x[i], cmp_cvt<T, ZP32>(y[i], zp, scale), l);
        }
    }
    const double sa = cmp_wave_fold(l.sa), sd = cmp_wave_fold(l.sd), sx = cmp_wave_fold(l.sx);
    if (lane == 0) {
      part[par][0][w] = sa;
      part[par][1][w] = sd;
      part[par][2][w] = sx;
    }
    // one barrier per chunk: part[par] is written again two chunks on, after the barrier of the
    // chunk between, which lane 0..2 reach only after reading it here
    __syncthreads();
    if (t < 3) scratch[t * nchunks + c] = (part[par][t][0] + part[par][t][1]) + (part[par][t][2] + part[par][t][3]);
  }
  // maximum and skips of everything this workgroup saw
  for (int off = 32; off > 0; off >>= 1) {
    const double o = __shfl_xor(l.mx, off, 64);
    l.mx = o > l.mx ? o : l.mx;
    l.skipped += __shfl_xor(l.skipped, off, 64);
  }
  if (lane == 0) {
    wmx[w] = l.mx;
    wskip[w] = l.skipped;
  }
  __syncthreads();
  if (t == 0) {
    double mx = wmx[0];
    uint64_t skipped = wskip[0];
    for (int i = 1; i < 4; ++i) {
      mx = wmx[i] > mx ? wmx[i] : mx;
      skipped += wskip[i];
    }
    unsigned long long* st = reinterpret_cast<unsigned long long*>(state);
    if (skipped) {  // pass 2 adds n to the compared count
      atomicAdd(st + 0, (unsigned long long)(0 - skipped));
      atomicAdd(st + 1, (unsigned long long)skipped);
    }
    const unsigned long long mb = (unsigned long long)__double_as_longlong(mx);
    if (mb > __hip_atomic_load(st + 5, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(st + 5, mb);
  }
}

// Pass 2: workgroup s of three takes sum s.  One workgroup reading ceil(n / 4096) doubles is
// bound by latency, not bytes (measured with one workgroup for all three sums and 16 loads in
// flight: 2 us per round of loads, 66 us of the 261 a [50432, 3072] pair took), hence a
// workgroup per sum and kCmpFinalUnroll loads in flight per lane before the first is added.
__global__ void __launch_bounds__(256)
k_cmp_final(const double* __restrict__ scratch, int64_t nchunks, int64_t n, int64_t* __restrict__ state) {
  __shared__ double part[4];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, s = blockIdx.x;
  const double* p = scratch + s * nchunks;
  double acc = 0.0;
  for (int64_t c0 = t; c0 < nchunks; c0 += 256 * kCmpFinalUnroll) {
    double v[kCmpFinalUnroll];
#pragma unroll
    for (int u = 0; u < kCmpFinalUnroll; ++u) {
      const int64_t c = c0 + 256 * u;
      v[u] = c < nchunks ? p[c] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < kCmpFinalUnroll; ++u) acc += v[u];  // + 0.0 past the end: nothing
  }
  acc = cmp_wave_fold(acc);
  if (lane == 0) part[w] = acc;
  __syncthreads();
  if (t == 0) {
    double* sf = reinterpret_cast<double*>(state);
    sf[2 + s] = sf[2 + s] + ((part[0] + part[1]) + (part[2] + part[3]));
    if (s == 0) state[0] += n;  // the skips were taken off by pass 1
  }
}

int cmp_cus() {
  static int n = 0;
  if (n == 0) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0)
      n = 256;
  }
  return n;
}

// workgroups of pass 1: NQK_CMP_GRID=<workgroups> (read on every call: the tests show with it
// that the state does not depend on the grid), else eight per CU
int64_t cmp_grid(int64_t nchunks) {
  const char* e = getenv("NQK_CMP_GRID");
  int64_t g = e && *e ? atoll(e) : 0;
  if (g < 1) g = (int64_t)8 * cmp_cus();
  // a workgroup counts its skips in 32 bits: at most 2^19 chunks (2^31 elements) each
  const int64_t least = (nchunks + ((int64_t)1 << 19) - 1) >> 19;
  if (g < least) g = least;
  return g < nchunks ? g : nchunks;
}

template <typename T, bool ZP32>
void launch_cmp(const float* x, const void* y, float scale, int64_t zp, int64_t n, int64_t nchunks, int64_t* state,
                double* scratch) {
  hipLaunchKernelGGL((k_cmp_chunks<T, ZP32>), dim3((unsigned)cmp_grid(nchunks)), dim3(256), 0, stream(), x,
                     (const T*)y, (double)scale, zp, n, nchunks, state, scratch);
}

}  // namespace
}  // namespace nqk

using namespace nqk;

extern "C" int nqk_compare_stats(const float* x, const void* y, int y_dtype, float scale, int64_t zp, int has_zp,
                                 int64_t n, int64_t* state, double* scratch, int64_t scratch_len) {
  if (n < 0) return fail("nqk_compare_stats: n < 0");
  if (n > NQK_CMP_MAX_N) return fail("nqk_compare_stats: n above NQK_CMP_MAX_N (2^36)");
  if (y_dtype != NQK_F32 && (y_dtype < NQK_I8 || y_dtype > NQK_I64))
    return fail("nqk_compare_stats: y_dtype is not f32 or an integer storage code");
  if (!x || !y || !state) return fail("nqk_compare_stats: null pointer");
  const int64_t nchunks = (n + kCmpChunk - 1) / kCmpChunk;
  if (scratch_len < 3 * nchunks) return fail("nqk_compare_stats: scratch shorter than 3 * ceil(n / 4096) doubles");
  if (n && !scratch) return fail("nqk_compare_stats: null pointer");
  const uintptr_t ysize = y_dtype == NQK_I8 ? 1 : y_dtype == NQK_I16 ? 2 : y_dtype == NQK_I64 ? 8 : 4;
  if ((uintptr_t)x % 4 || (uintptr_t)y % ysize || (uintptr_t)state % 8 || (uintptr_t)scratch % 8)
    return fail("nqk_compare_stats: x and y need the alignment of their elements, state and scratch 8 bytes");
  if (n == 0) return 0;
  const int64_t z = has_zp ? zp : 0;
  const bool z32 = z >= -((int64_t)1 << 30) && z <= ((int64_t)1 << 30);
  switch (y_dtype) {
    case NQK_F32: launch_cmp<float, false>(x, y, 1.0f, 0, n, nchunks, state, scratch); break;
    case NQK_I8:
      if (z32) launch_cmp<int8_t, true>(x, y, scale, z, n, nchunks, state, scratch);
      else launch_cmp<int8_t, false>(x, y, scale, z, n, nchunks, state, scratch);
      break;
    case NQK_I16:
      if (z32) launch_cmp<int16_t, true>(x, y, scale, z, n, nchunks, state, scratch);
      else launch_cmp<int16_t, false>(x, y, scale, z, n, nchunks, state, scratch);
      break;
    case NQK_I32: launch_cmp<int32_t, false>(x, y, scale, z, n, nchunks, state, scratch); break;
    default: launch_cmp<int64_t, false>(x, y, scale, z, n, nchunks, state, scratch); break;
  }
  hipLaunchKernelGGL(k_cmp_final, dim3(3), dim3(256), 0, stream(), (const double*)scratch, nchunks, n, state);
  return launch_status("nqk_compare_stats");
}
