// Per-token (per-row) activation quantization (Model.quantize(per_token=True)): the row quantizer
// and the int8 MFMA GEMM whose epilogue applies the rank-one scale s[m] * sw[n].
//
// Arithmetic (include/nqk.h states it; tests/_per_token_ref.py is its NumPy restatement).  Row m of
// x [rows][cols]:
//   lo = min(min_k x, 0), hi = max(max_k x, 0)
//   s = f32(f32(hi - lo) / f32(2^bw - 1));  z = rint(f32(qlo - f32(lo / s)))     quant_parameters
//   s == 0 (an all-zero row, a range that underflows): s = 1, z = 0, every q = 0
//   q[k] = int(rint(clip(f64(z) + f64(f32(x[k] / s)), qlo, qhi)))                nqk_quantize, has_zp
// and the product with a symmetric weight bt [N][K] (column scales sw, column sums colsum):
//   P = sum_k q[m][k] bt[n][k]                                                   exact, int32
//   out[m][n] = f32(f64(P - z[m] colsum[n]) * f64(f32(s[m] * sw[n])))
// |P - z colsum| <= 255 * 128 * K < 2^31 for K < 2^16; a longer K is refused.
//
// nqk_quantize_rows reads x from HBM once.  One wave owns a row and keeps it in registers: float4
// chunk c = lane + 64 i, i < 16, so up to 4096 columns; a 256-thread workgroup takes 4 rows and
// needs no barrier.  min and max are order-free, so the cross-lane butterfly is exact.  Every lane
// then holds s and z, quantizes its registers with the IEEE divide and stores 4 packed bytes per
// chunk; the bytes from cols up to ldq are written as 0, which is nqk_qgemm_i8's K padding.  A
// row whose address is not 16-byte aligned, and the last partial chunk, load element by element;
// elements past cols read as 0, which changes neither lo nor hi.  Rows longer than 4096 take
// k_quantize_rows_long: a workgroup per row, one pass for the range and a second, served by L2,
// that quantizes.
//
// nqk_qgemm_rows is k_qgemm_i8's frame (nqk_gemm.hip): 128 x 128 x 64 tile, 4 waves (2 x 2, 64 x 64
// each = 2 x 2 tiles of v_mfma_i32_32x32x32_i8), double-buffered LDS with its 16-byte chunk swizzle.
// In the 32 x 32 C/D layout a lane holds one column per MFMA tile: sw[n] and colsum[n] are two
// registers per column tile, loaded before the k loop.  The tile's 128 (s, z) pairs are read from
// global memory while the last k-tile computes and stored to 1 KiB of LDS before that tile's
// barrier; the epilogue reads the pair of its row as a broadcast.  Per output: v_mul_f32, an
// integer multiply-subtract, two conversions to f64, v_mul_f64, v_cvt_f32_f64, one f32 store.  No
// integer [M][N] array exists.
#include "nqk_common.h"

namespace nqk {
namespace {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));

// ------------------------------------------------------------------------------- row quantizer
constexpr int QR_CHUNKS = 16;             // float4 chunks a lane keeps
constexpr int QR_REG_COLS = 64 * 4 * QR_CHUNKS;  // 4096

// chunk c (columns 4c .. 4c + 3) of a row; columns past `cols` read as 0
__device__ __forceinline__ float4 load_chunk(const float* __restrict__ xr, int64_t c, int64_t cols, bool vec) {
  const int64_t k = 4 * c;
  if (vec && k + 3 < cols) return *reinterpret_cast<const float4*>(xr + k);
  float4 v = {0.0f, 0.0f, 0.0f, 0.0f};
  if (k < cols) v.x = xr[k];
  if (k + 1 < cols) v.y = xr[k + 1];
  if (k + 2 < cols) v.z = xr[k + 2];
  if (k + 3 < cols) v.w = xr[k + 3];
  return v;
}

__device__ __forceinline__ void minmax4(const float4& v, float& mn, float& mx) {
  mn = __builtin_fminf(__builtin_fminf(mn, v.x), __builtin_fminf(v.y, __builtin_fminf(v.z, v.w)));
  mx = __builtin_fmaxf(__builtin_fmaxf(mx, v.x), __builtin_fmaxf(v.y, __builtin_fmaxf(v.z, v.w)));
}

__device__ __forceinline__ void wave_minmax(float& mn, float& mx) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    mn = __builtin_fminf(mn, __shfl_xor(mn, off, 64));
    mx = __builtin_fmaxf(mx, __shfl_xor(mx, off, 64));
  }
}

struct RowP {
  float s;
  int z;
};

// quant_parameters(lo, hi, bw, asymmetric=True) in float32; span = 2^bw - 1, qlo = -2^(bw-1)
__device__ __forceinline__ RowP row_params(float mn, float mx, float span, float qlo) {
  const float lo = __builtin_fminf(mn, 0.0f), hi = __builtin_fmaxf(mx, 0.0f);
  RowP p;
  p.s = (hi - lo) / span;
  p.z = 0;
  if (p.s == 0.0f) p.s = 1.0f;
  else p.z = (int)__builtin_rintf(qlo - lo / p.s);
  return p;
}

__device__ __forceinline__ uint32_t quant_byte(float x, float s, double z, double lo, double hi) {
  const float t = x / s;  // correctly rounded
  double u = z + (double)t;
  u = u < lo ? lo : u;
  u = u > hi ? hi : u;
  return (uint32_t)(int)__builtin_rint(u) & 255u;
}

// the 4 bytes of chunk c; bytes of columns past `cols` are 0
__device__ __forceinline__ uint32_t quant_chunk(const float4& v, int64_t c, int64_t cols, float s, double z, double lo,
                                                double hi) {
  const int64_t k = 4 * c;
  uint32_t w = quant_byte(v.x, s, z, lo, hi);
  if (k + 1 < cols) w |= quant_byte(v.y, s, z, lo, hi) << 8;
  if (k + 2 < cols) w |= quant_byte(v.z, s, z, lo, hi) << 16;
  if (k + 3 < cols) w |= quant_byte(v.w, s, z, lo, hi) << 24;
  return w;
}

// zero bytes from the first chunk past cols up to ldq, `step` threads starting at `t`
__device__ __forceinline__ void zero_pad(int8_t* __restrict__ qr, int64_t cols, int64_t ldq, int t, int step) {
  for (int64_t c = ((cols + 3) >> 2) + t; c < (ldq >> 2); c += step) *reinterpret_cast<uint32_t*>(qr + 4 * c) = 0u;
}

__global__ void __launch_bounds__(256)
k_quantize_rows_reg(const float* __restrict__ x, int8_t* __restrict__ q, float* __restrict__ s, int32_t* __restrict__ z,
                    int64_t rows, int64_t cols, int64_t ldx, int64_t ldq, float span, float qlo, float qhi) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;  // no barrier below
  const float* xr = x + row * ldx;
  int8_t* qr = q + row * ldq;
  const bool vec = (((uintptr_t)xr) & 15) == 0;
  float4 v[QR_CHUNKS];
  float mn = 0.0f, mx = 0.0f;  // 0 belongs to the range
#pragma unroll
  for (int i = 0; i < QR_CHUNKS; ++i) {
    v[i] = float4{0.0f, 0.0f, 0.0f, 0.0f};
    if ((int64_t)i * 256 < cols) {  // wave-uniform
      v[i] = load_chunk(xr, lane + 64 * i, cols, vec);
      minmax4(v[i], mn, mx);
    }
  }
  wave_minmax(mn, mx);
  const RowP p = row_params(mn, mx, span, qlo);
  const double zd = (double)p.z, lo = (double)qlo, hi = (double)qhi;
#pragma unroll
  for (int i = 0; i < QR_CHUNKS; ++i) {
    const int64_t c = lane + 64 * i;
    if ((int64_t)i * 256 < cols && 4 * c < cols)
      *reinterpret_cast<uint32_t*>(qr + 4 * c) = quant_chunk(v[i], c, cols, p.s, zd, lo, hi);
  }
  zero_pad(qr, cols, ldq, lane, 64);
  if (lane == 0) {
    s[row] = p.s;
    z[row] = p.z;
  }
}

__global__ void __launch_bounds__(256)
k_quantize_rows_long(const float* __restrict__ x, int8_t* __restrict__ q, float* __restrict__ s,
                     int32_t* __restrict__ z, int64_t cols, int64_t ldx, int64_t ldq, float span, float qlo,
                     float qhi) {
  __shared__ float smn[4], smx[4];
  const int tid = threadIdx.x;
  const int64_t row = blockIdx.x;
  const float* xr = x + row * ldx;
  int8_t* qr = q + row * ldq;
  const bool vec = (((uintptr_t)xr) & 15) == 0;
  const int64_t nchunks = (cols + 3) >> 2;
  float mn = 0.0f, mx = 0.0f;
  for (int64_t c = tid; c < nchunks; c += 256) minmax4(load_chunk(xr, c, cols, vec), mn, mx);
  wave_minmax(mn, mx);
  if ((tid & 63) == 0) {
    smn[tid >> 6] = mn;
    smx[tid >> 6] = mx;
  }
  __syncthreads();
  mn = __builtin_fminf(__builtin_fminf(smn[0], smn[1]), __builtin_fminf(smn[2], smn[3]));
  mx = __builtin_fmaxf(__builtin_fmaxf(smx[0], smx[1]), __builtin_fmaxf(smx[2], smx[3]));
  const RowP p = row_params(mn, mx, span, qlo);
  const double zd = (double)p.z, lo = (double)qlo, hi = (double)qhi;
  for (int64_t c = tid; c < nchunks; c += 256)
    *reinterpret_cast<uint32_t*>(qr + 4 * c) = quant_chunk(load_chunk(xr, c, cols, vec), c, cols, p.s, zd, lo, hi);
  zero_pad(qr, cols, ldq, tid, 256);
  if (tid == 0) {
    s[row] = p.s;
    z[row] = p.z;
  }
}

// ------------------------------------------------------------------------------- row-scaled GEMM
constexpr int BM = 128, BN = 128, BK = 64;

struct SZ {  // a row's scale and zero point, one ds_read_b64
  float s;
  int z;
};

__global__ void __launch_bounds__(256)
k_qgemm_rows(const int8_t* __restrict__ A, const int8_t* __restrict__ Bt, const float* __restrict__ S,
             const int32_t* __restrict__ Z, const float* __restrict__ sw, const int64_t* __restrict__ colsum,
             float* __restrict__ C, int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldb, int64_t ldc,
             int tiles_n) {
  __shared__ __attribute__((aligned(16))) int8_t smem[2 * (BM + BN) * BK];
  __shared__ __attribute__((aligned(16))) SZ rowp[BM];
#define AS(buf) (smem + (buf) * (BM + BN) * BK)
#define BS(buf) (smem + (buf) * (BM + BN) * BK + BM * BK)

  const int tm = blockIdx.x / tiles_n, tn = blockIdx.x % tiles_n;
  const int64_t m0 = (int64_t)tm * BM, n0 = (int64_t)tn * BN;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int r32 = lane & 31, half = lane >> 5;

  // staging: 512 chunks of 16 B per operand tile, 2 per thread (K % 16 == 0: a chunk lies inside K
  // or outside it; outside reads as zeros)
  v4i ra[2], rb[2];
  auto load_tile = [&](int64_t k0) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int idx = tid + i * 256, row = idx >> 2, ch = idx & 3;
      const int64_t kk = k0 + ch * 16;
      const int64_t gm = m0 + row, gn = n0 + row;
      const v4i zero = {0, 0, 0, 0};
      ra[i] = (gm < M && kk < K) ? *reinterpret_cast<const v4i*>(A + gm * lda + kk) : zero;
      rb[i] = (gn < N && kk < K) ? *reinterpret_cast<const v4i*>(Bt + gn * ldb + kk) : zero;
    }
  };
  auto store_tile = [&](int buf) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int idx = tid + i * 256, off = swz(idx >> 2, idx & 3);
      *reinterpret_cast<v4i*>(AS(buf) + off) = ra[i];
      *reinterpret_cast<v4i*>(BS(buf) + off) = rb[i];
    }
  };

  // the lane's two columns: their weight scale and column sum (0 past N: never stored)
  int64_t gcol[2];
  float swj[2];
  int csj[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    gcol[j] = n0 + wn * 64 + j * 32 + r32;
    const bool ok = gcol[j] < N;
    swj[j] = ok ? sw[gcol[j]] : 0.0f;
    csj[j] = ok ? (int)colsum[gcol[j]] : 0;
  }

  v16i acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0;

  const int nk = (int)((K + BK - 1) / BK);
  load_tile(0);
  store_tile(0);
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const int cur = kt & 1;
    const bool last = kt + 1 == nk;
    SZ mine = {1.0f, 0};
    if (!last) load_tile((int64_t)(kt + 1) * BK);
    else if (tid < BM && m0 + tid < M) mine = SZ{S[m0 + tid], Z[m0 + tid]};  // in flight under the MFMAs
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      v4i fa[2], fb[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) fa[i] = *reinterpret_cast<const v4i*>(AS(cur) + swz(wm * 64 + i * 32 + r32, 2 * s + half));
#pragma unroll
      for (int j = 0; j < 2; ++j) fb[j] = *reinterpret_cast<const v4i*>(BS(cur) + swz(wn * 64 + j * 32 + r32, 2 * s + half));
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(fa[i], fb[j], acc[i][j], 0, 0, 0);
    }
    if (!last) store_tile(cur ^ 1);
    else if (tid < BM) rowp[tid] = mine;
    __syncthreads();
  }

  // C/D layout (gfx950, dtype independent): col = lane & 31, row = (r&3) + 8*(r>>2) + 4*(lane>>5)
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int rl = wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
      const SZ p = rowp[rl];
      const int64_t gm = m0 + rl;
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const float sc = p.s * swj[j];
        const int v = acc[i][j][r] - p.z * csj[j];
        if (gm < M && gcol[j] < N) C[gm * ldc + gcol[j]] = (float)((double)v * (double)sc);
      }
    }
#undef AS
#undef BS
}

}  // namespace
}  // namespace nqk

using namespace nqk;

static bool misaligned(const void* p, uintptr_t a) { return !p || (((uintptr_t)p) & (a - 1)); }

extern "C" int nqk_quantize_rows(const float* x, int8_t* q, float* s, int32_t* z, int64_t rows, int64_t cols,
                                 int64_t ldx, int64_t ldq, int bit_width) {
  const std::string who = "nqk_quantize_rows";
  if (bit_width < 2 || bit_width > 8) return fail(who + ": bit_width must lie in 2..8 (int8 storage)");
  if (rows < 0 || cols <= 0) return fail(who + ": rows must not be negative and cols must be positive");
  if (ldx < cols) return fail(who + ": ldx is shorter than a row");
  if (ldq < cols || (ldq & 15)) return fail(who + ": ldq must be a multiple of 16 and at least cols");
  if (misaligned(x, 4) || misaligned(s, 4) || misaligned(z, 4)) return fail(who + ": x, s and z must be 4-byte aligned pointers");
  if (misaligned(q, 16)) return fail(who + ": q must be a 16-byte aligned pointer");
  if (rows == 0) return 0;
  if (rows > 0x7fffffff) return fail(who + ": too many rows");
  const float qlo = -(float)(1 << (bit_width - 1)), qhi = (float)((1 << (bit_width - 1)) - 1);
  const float span = (float)((1 << bit_width) - 1);
  if (cols <= QR_REG_COLS)
    hipLaunchKernelGGL(k_quantize_rows_reg, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, stream(), x, q, s, z, rows,
                       cols, ldx, ldq, span, qlo, qhi);
  else
    hipLaunchKernelGGL(k_quantize_rows_long, dim3((unsigned)rows), dim3(256), 0, stream(), x, q, s, z, cols, ldx, ldq,
                       span, qlo, qhi);
  return launch_status(who.c_str());
}

extern "C" int nqk_qgemm_rows(const int8_t* a, const int8_t* bt, const float* s, const int32_t* z, const float* sw,
                              const int64_t* colsum, float* out, int64_t M, int64_t N, int64_t K, int64_t lda,
                              int64_t ldb, int64_t ldo) {
  const std::string who = "nqk_qgemm_rows";
  if (K <= 0 || (K & 15)) return fail(who + ": K must be a positive multiple of 16");
  if (K >= (1 << 16)) return fail(who + ": K of 65536 or more can overflow the int32 P - z colsum");
  if (N <= 0) return fail(who + ": N must be positive");
  if ((ldb & 15) || ldb < K) return fail(who + ": ldb must be a multiple of 16 and at least K");
  if (misaligned(bt, 16)) return fail(who + ": bt must be a 16-byte aligned pointer");
  if (M <= 0) return 0;
  if ((lda & 15) || lda < K) return fail(who + ": lda must be a multiple of 16 and at least K");
  if (ldo < N) return fail(who + ": ldo is shorter than a row of the output");
  if (misaligned(a, 16)) return fail(who + ": a must be a 16-byte aligned pointer");
  if (misaligned(s, 4) || misaligned(z, 4) || misaligned(sw, 4) || misaligned(out, 4))
    return fail(who + ": s, z, sw and out must be 4-byte aligned pointers");
  if (misaligned(colsum, 8)) return fail(who + ": colsum must be an 8-byte aligned pointer");
  const int64_t tiles_m = (M + BM - 1) / BM, tiles_n = (N + BN - 1) / BN;
  if (tiles_m * tiles_n > 0x7fffffff) return fail(who + ": too many tiles");
  hipLaunchKernelGGL(k_qgemm_rows, dim3((unsigned)(tiles_m * tiles_n)), dim3(256), 0, stream(), a, bt, s, z, sw, colsum,
                     out, M, N, K, lda, ldb, ldo, (int)tiles_n);
  return launch_status(who.c_str());
}
