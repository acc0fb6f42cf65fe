// Top-k classes and their Softmax probabilities of every row, in one pass over the row
// (QModel.classify: the step after the classifier Gemm, which the reference leaves to its
// callers as np.argsort / np.exp on the host).
//
// The row y is x itself (f32) or the dequantized integer row f32(f64(q - zp) * f64(s))
// (numpy_quantization.py:37-41, the expression of k_dequantize), and per row
//   idx   = np.argsort(-y, kind="stable")[:k]
//   value = y[idx]
//   prob  = Softmax(y)[idx] with the bits of nqk_softmax_lastdim (k_softmax, nqk_float.hip):
//           the same row max, np_expf(y + (-max)), NumPy's pairwise sum through the same
//           PwPlan, one IEEE divide per selected element.
// One wave per row, rows grid-stride; the row is read from memory once (16-byte loads when the
// rows are aligned, several in flight per lane) into the wave's LDS slice, and everything after
// that (selection, exp, sum) works on LDS.
//
// Ordering: a total order on (NaN last, larger value first with -0 == +0, lower column
// first) packed into one uint64 key per element, larger key = earlier in the output:
//   high word  0 for NaN, else the usual monotone map of the float's bits (-0 read as +0);
//              every number maps above 0, so NaNs sort after all of them
//   low word   0xFFFFFFFF - column, so equal values (and NaNs) go by increasing column
// Keys are distinct within a row.  Every lane keeps the two largest keys of its own columns.
// Round j takes the wave-wide maximum of the lanes' best remaining keys; the lane that owned
// the winner moves its runner-up up, and only when it wins again after that does it read its
// columns again for its two largest keys below the winner (everything above a winner has been
// selected before it).  Nothing is struck out in LDS, so the row stays intact for the exp pass.
#include "nqk_common.h"
#include "nqk_numerics.h"

namespace nqk {
namespace {

constexpr int kTopkMaxK = 64;        // one winner per lane
constexpr int kTopkMaxBlocks = 1024;  // rows beyond grid * waves are taken grid-stride

template <typename T>
__device__ __forceinline__ float topk_cvt(T q, int64_t zp, double scale) {
  return (float)((double)((int64_t)q - zp) * scale);  // k_dequantize, scalar or no zero point
}
template <>
__device__ __forceinline__ float topk_cvt<float>(float y, int64_t, double) { return y; }

__device__ __forceinline__ uint64_t topk_key(float y, int col) {
  uint32_t u = __float_as_uint(y), ord = 0;
  if (y == y) {
    if (y == 0.0f) u = 0;  // -0 ties with +0
    ord = (u >> 31) ? ~u : (u | 0x80000000u);
  }
  return ((uint64_t)ord << 32) | (uint64_t)(0xFFFFFFFFu - (uint32_t)col);
}
// keep the two largest of the keys seen: best >= second
__device__ __forceinline__ void topk_push(uint64_t key, uint64_t& best, uint64_t& second) {
  const uint64_t lower = key < best ? key : best;
  second = lower > second ? lower : second;
  best = key > best ? key : best;
}
__device__ __forceinline__ int topk_col(uint64_t key) { return (int)(0xFFFFFFFFu - (uint32_t)key); }

// Wave-wide maximum, the same in every lane.  Inside a row of 16 lanes by DPP: the two quad
// exchanges, then row_half_mirror and row_mirror (a maximum may meet a lane twice); across
// the four rows by v_readlane.  All 64 lanes must be active.
template <int CTRL>
__device__ __forceinline__ uint32_t dpp_u32(uint32_t x) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, CTRL, 0xF, 0xF, false);
}
template <int CTRL>
__device__ __forceinline__ uint64_t dpp_u64(uint64_t x) {
  return ((uint64_t)dpp_u32<CTRL>((uint32_t)(x >> 32)) << 32) | dpp_u32<CTRL>((uint32_t)x);
}
__device__ __forceinline__ uint64_t readlane_u64(uint64_t x, int lane) {
  return ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(x >> 32), lane) << 32) |
         (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)x, lane);
}
constexpr int kDppQuadXor1 = 0xB1, kDppQuadXor2 = 0x4E, kDppRowHalfMirror = 0x141, kDppRowMirror = 0x140;
__device__ __forceinline__ uint64_t wave_max_u64(uint64_t x) {
  uint64_t o;
  o = dpp_u64<kDppQuadXor1>(x);      x = o > x ? o : x;
  o = dpp_u64<kDppQuadXor2>(x);      x = o > x ? o : x;
  o = dpp_u64<kDppRowHalfMirror>(x); x = o > x ? o : x;
  o = dpp_u64<kDppRowMirror>(x);     x = o > x ? o : x;
  uint64_t a = readlane_u64(x, 0), c = readlane_u64(x, 32);
  const uint64_t b = readlane_u64(x, 16), d = readlane_u64(x, 48);
  a = b > a ? b : a;
  c = d > c ? d : c;
  return c > a ? c : a;
}
// k_softmax's row maximum (`o > mx ? o : mx`, NaNs never taken).  The order of the comparisons
// differs from its butterfly, which can only change the sign of a zero maximum, and
// np_expf(y + -0) == np_expf(y + +0) for every y that is not larger than that maximum.
__device__ __forceinline__ float wave_max_f32(float x) {
  float o;
  o = __uint_as_float(dpp_u32<kDppQuadXor1>(__float_as_uint(x)));      x = o > x ? o : x;
  o = __uint_as_float(dpp_u32<kDppQuadXor2>(__float_as_uint(x)));      x = o > x ? o : x;
  o = __uint_as_float(dpp_u32<kDppRowHalfMirror>(__float_as_uint(x))); x = o > x ? o : x;
  o = __uint_as_float(dpp_u32<kDppRowMirror>(__float_as_uint(x)));     x = o > x ? o : x;
  float a = __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(x), 0));
  float c = __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(x), 32));
  const float b = __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(x), 16));
  const float d = __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(x), 48));
  a = b > a ? b : a;
  c = d > c ? d : c;
  return c > a ? c : a;
}

// V consecutive elements as one access (V = 4: 16 bytes of f32 / int32, 4 of int8, ...)
template <typename T, int V>
struct alignas(V * sizeof(T) > 16 ? 16 : V * sizeof(T)) Pack {
  T e[V];
};

// blockDim.x / 64 waves per block, one row per wave; `slice` floats of LDS per wave.  The row
// is cut into groups of V columns; group g belongs to lane g % 64, which loads it, keeps its
// best remaining keys and reads it again when they run out.  V = 4 needs cols % 4 == 0 and rows
// aligned to the Pack (the launcher checks); V = 1 takes everything else.  U groups per lane are
// loaded before the first is used, so a row costs one or two memory latencies, not one per
// element.
template <typename T, int V>
__global__ void __launch_bounds__(256)
k_topk_softmax(const T* __restrict__ x, double scale, int64_t zp, int64_t rows, int cols, int64_t ldx, int k,
               int64_t* __restrict__ idx, float* __restrict__ prob, float* __restrict__ value, PwPlan p, int slice) {
  constexpr int U = V == 1 ? 8 : 4;
  using PT = Pack<T, V>;
  using PF = Pack<float, V>;
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, wpb = blockDim.x >> 6;
  float* v = sm + w * slice;
  float* part = v + cols;
  float* leafv = part + kMaxLeaves * 8;
  const int ngroup = cols / V;
  for (int64_t r = (int64_t)blockIdx.x * wpb + w; r < rows; r += (int64_t)gridDim.x * wpb) {
    const T* xr = x + r * ldx;
    float mx = -__builtin_inff();
    // the two largest keys of this lane's columns not yet selected (0: none left); after a win
    // the runner-up moves up and the next one is unknown until the lane wins again (have2)
    uint64_t best = 0, second = 0;
    bool have2 = true;
    for (int g0 = lane; g0 < ngroup; g0 += 64 * U) {
      PT raw[U] = {};
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int g = g0 + 64 * u;
        if (g < ngroup) raw[u] = *reinterpret_cast<const PT*>(xr + (int64_t)g * V);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int g = g0 + 64 * u;
        if (g < ngroup) {
          PF f;
#pragma unroll
          for (int e = 0; e < V; ++e) {
            const float t = topk_cvt<T>(raw[u].e[e], zp, scale);
            f.e[e] = t;
            mx = t > mx ? t : mx;
            topk_push(topk_key(t, g * V + e), best, second);
          }
          *reinterpret_cast<PF*>(v + g * V) = f;
        }
      }
    }
    mx = wave_max_f32(mx);
    wave_lds_sync();
    uint64_t mine = 0;  // lane j keeps the winner of round j
    for (int j = 0; j < k; ++j) {
      const uint64_t win = wave_max_u64(best);
      if (lane == j) mine = win;
      if (lane == ((topk_col(win) / V) & 63)) {  // the owner: what it has left lies below the winner
        if (have2) {
          best = second;
          have2 = false;
        } else {  // it won again and has no runner-up: read its columns again
          best = second = 0;
          for (int g = lane; g < ngroup; g += 64) {
            const PF f = *reinterpret_cast<const PF*>(v + g * V);
#pragma unroll
            for (int e = 0; e < V; ++e) {
              const uint64_t key = topk_key(f.e[e], g * V + e);
              if (key < win) topk_push(key, best, second);
            }
          }
          have2 = true;
        }
      }
    }
    int col = 0;
    float val = 0.0f;
    if (lane < k) {
      col = topk_col(mine);
      if (mine == 0 || col >= cols) col = 0;  // cannot happen for k <= cols; keeps the LDS read in range
      val = v[col];
    }
    if (prob) {
      const float nm = -mx;
      for (int g = lane; g < ngroup; g += 64) {
        PF f = *reinterpret_cast<const PF*>(v + g * V);
#pragma unroll
        for (int e = 0; e < V; ++e) f.e[e] = np_expf(f.e[e] + nm);
        *reinterpret_cast<PF*>(v + g * V) = f;
      }
      wave_lds_sync();
      const float s = wave_pairwise_sum(v, p, part, leafv);
      if (lane < k) prob[r * k + lane] = v[col] / s;
    }
    if (lane < k) {
      idx[r * k + lane] = col;
      if (value) value[r * k + lane] = val;
    }
    wave_lds_sync();
  }
}

template <typename T>
void launch_topk(const void* x, float scale, int64_t zp, int64_t rows, int64_t cols, int64_t ldx, int k, int64_t* idx,
                 float* prob, float* value, const PwPlan& p) {
  const int64_t slice = (int64_t)(row_smem(cols) / sizeof(float) + 3) / 4 * 4;
  // four rows per block while their slices fit 64 KiB of LDS; longer rows one wave per block
  const int wpb = 4 * slice * (int64_t)sizeof(float) <= (64 << 10) ? 4 : 1;
  const int64_t want = (rows + wpb - 1) / wpb;
  const dim3 grid((unsigned)(want < kTopkMaxBlocks ? want : kTopkMaxBlocks)), block(64 * wpb);
  const size_t lds = (size_t)wpb * slice * sizeof(float);
  const bool packs = cols % 4 == 0 && ldx % 4 == 0 && (uintptr_t)x % alignof(Pack<T, 4>) == 0;
  if (packs)
    hipLaunchKernelGGL((k_topk_softmax<T, 4>), grid, block, lds, stream(), (const T*)x, (double)scale, zp, rows,
                       (int)cols, ldx, k, idx, prob, value, p, (int)slice);
  else
    hipLaunchKernelGGL((k_topk_softmax<T, 1>), grid, block, lds, stream(), (const T*)x, (double)scale, zp, rows,
                       (int)cols, ldx, k, idx, prob, value, p, (int)slice);
}

}  // namespace
}  // namespace nqk

using namespace nqk;

extern "C" int nqk_topk_softmax(const void* x, int x_dtype, float scale, int64_t zp, int has_zp, int64_t rows,
                                int64_t cols, int64_t ldx, int k, int64_t* idx, float* prob, float* value) {
  if (rows < 0) return fail("nqk_topk_softmax: rows < 0");
  if (cols < 1) return fail("nqk_topk_softmax: cols < 1");
  if (cols > 8192) return fail("nqk_topk_softmax: cols > 8192 (the pairwise-sum plan's limit)");
  if (k < 1 || k > cols || k > kTopkMaxK) return fail("nqk_topk_softmax: k outside 1..min(cols, 64)");
  if (ldx < cols) return fail("nqk_topk_softmax: ldx < cols");
  if (x_dtype != NQK_F32 && (x_dtype < NQK_I8 || x_dtype > NQK_I64))
    return fail("nqk_topk_softmax: x_dtype is not f32 or an integer storage code");
  if (rows == 0) return 0;
  if (!x || !idx) return fail("nqk_topk_softmax: null pointer");
  PwPlan p;
  if (row_plan(cols, p)) return -1;
  if (x_dtype == NQK_F32) {
    launch_topk<float>(x, 1.0f, 0, rows, cols, ldx, k, idx, prob, value, p);
  } else {
    const int64_t z = has_zp ? zp : 0;
    NQK_INT_DISPATCH(x_dtype, T, launch_topk<T>(x, scale, z, rows, cols, ldx, k, idx, prob, value, p));
  }
  return launch_status("nqk_topk_softmax");
}
