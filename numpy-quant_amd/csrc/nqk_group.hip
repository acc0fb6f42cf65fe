// nqk_qgemm_group — int8 MFMA GEMM for a weight with one scale per group of g consecutive k and
// column (Model.quantize(group_size=g)).  The rescale sits inside the k loop: no integer [M][N]
// array exists, the float32 result is written directly.
//
// Arithmetic (include/nqk.h states it; tests/_group_ref.py is its NumPy restatement), per output:
//   P_j  = sum_{k in group j} a[m][k] b[n][k] - zpa gsum[j][n]          exact, int32
//   acc  = 0.0 (f64); for j = 0 .. G-1 in order: acc = acc + f64(sg[j][n]) * f64(P_j)
//   out  = f32(acc)
// f64(sg) * f64(P_j) is exact while it has at most 53 significant bits: sg has 24, so P_j may
// have 29, |P_j| <= 255 * 128 * g < 2^29, which holds for g <= 16384; both entries refuse a larger
// g.  An exact product makes v_fma_f64 bit-equal to multiply-then-add: the only roundings are the
// G - 1 f64 additions, in order, and the final f32 conversion.  The fma is written explicitly (the
// tree is built -ffp-contract=off).  int32 wrap-around inside a group is harmless: P_j itself fits.
//
// Frame: k_qgemm_i8's (nqk_gemm.hip).  128 x 128 x 64 tile, 4 waves (2 x 2, 64 x 64 each = 2 x 2
// tiles of v_mfma_i32_32x32x32_i8), double-buffered LDS with its 16-byte chunk swizzle,
// ds_read_b128 fragments.  A k-tile is two k-steps of 32; a group is g / 32 k-steps, so a group
// may end in the middle of a k-tile.
//
// In the 32 x 32 C/D layout a lane holds one column per MFMA tile: sg[j][n] and -zpa gsum[j][n]
// are one value per lane and column tile.  A group's int32 accumulators start at -zpa gsum[j][n]
// (they have to be reset anyway), so the zero-point term costs nothing in the loop.  Both values
// of group j + 1 are loaded while group j runs.
//
// Group boundary: per accumulator element one v_cvt_f64_i32 and one v_fma_f64 into the resident
// f64 accumulator, 128 VALU instructions per wave against 4 g / 32 MFMAs, then the reset.  One int32
// accumulator set: the form with two alternating sets (group j + 1's MFMAs issued before group j is
// drained) measured 3 to 9 % slower at every shape and group size: it needs 485
// registers and moves accumulators between the two register files.
#include "nqk_common.h"

namespace nqk {
namespace {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));

constexpr int BM = 128, BN = 128, BK = 64;

__global__ void __launch_bounds__(256)
k_qgemm_group(const int8_t* __restrict__ A, const int8_t* __restrict__ Bt, const float* __restrict__ sg,
              const int32_t* __restrict__ gsum, float* __restrict__ C, int64_t M, int64_t N, int64_t K, int64_t lda,
              int64_t ldb, int64_t ldc, int spg /* k-steps of 32 per group */, int G, int zpa, int tiles_n) {
  __shared__ __attribute__((aligned(16))) int8_t smem[2 * (BM + BN) * BK];
#define AS(buf) (smem + (buf) * (BM + BN) * BK)
#define BS(buf) (smem + (buf) * (BM + BN) * BK + BM * BK)

  const int tm = blockIdx.x / tiles_n, tn = blockIdx.x % tiles_n;
  const int64_t m0 = (int64_t)tm * BM, n0 = (int64_t)tn * BN;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int r32 = lane & 31, half = lane >> 5;

  // staging: 512 chunks of 16 B per operand tile, 2 per thread (K % 32 == 0: a chunk lies inside K
  // or outside it; outside reads as zeros, which add nothing to P_j)
  v4i ra[2], rb[2];
  auto load_tile = [&](int64_t k0) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int idx = tid + i * 256, row = idx >> 2, ch = idx & 3;
      const int64_t kk = k0 + ch * 16;
      const int64_t gm = m0 + row, gn = n0 + row;
      const v4i z = {0, 0, 0, 0};
      ra[i] = (gm < M && kk < K) ? *reinterpret_cast<const v4i*>(A + gm * lda + kk) : z;
      rb[i] = (gn < N && kk < K) ? *reinterpret_cast<const v4i*>(Bt + gn * ldb + kk) : z;
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

  // the lane's two columns; what group jg starts from and is scaled by (0 past N)
  int64_t gcol[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) gcol[j] = n0 + wn * 64 + j * 32 + r32;
  int ninit[2];
  float nsg[2];
  auto load_group = [&](int jg) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const bool ok = jg < G && gcol[j] < N;
      const int64_t at = (int64_t)jg * N + gcol[j];
      nsg[j] = ok ? sg[at] : 0.0f;
      ninit[j] = (ok && gsum) ? -zpa * gsum[at] : 0;
    }
  };

  v16i acc[2][2];  // [row tile][column tile]
  float sgs[2];    // [column tile]: the scale of the running group
  double facc[2][2][16];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) facc[i][j][r] = 0.0;

  auto begin = [&](int jg) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      sgs[j] = nsg[j];
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][j][r] = ninit[j];
    }
    load_group(jg + 1);
  };
  // acc = fma(f64(sg), f64(P_j), acc): the product is exact (header), so this is
  // acc + f64(sg) * f64(P_j) with its one rounding, the restatement's multiply-then-add
  auto drain = [&]() {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const double s = (double)sgs[j];
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) facc[i][j][r] = __builtin_fma(s, (double)acc[i][j][r], facc[i][j][r]);
    }
  };

  const int nk = (int)((K + BK - 1) / BK);
  // k-step ks: 32 k, half a k-tile
  auto kstep = [&](int ks) {
    const int kt = ks >> 1, s = ks & 1, cur = kt & 1;
    if (s == 0 && kt + 1 < nk) load_tile((int64_t)(kt + 1) * BK);
    v4i fa[2], fb[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) fa[i] = *reinterpret_cast<const v4i*>(AS(cur) + swz(wm * 64 + i * 32 + r32, 2 * s + half));
#pragma unroll
    for (int j = 0; j < 2; ++j) fb[j] = *reinterpret_cast<const v4i*>(BS(cur) + swz(wn * 64 + j * 32 + r32, 2 * s + half));
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(fa[i], fb[j], acc[i][j], 0, 0, 0);
    if (s == 1) {
      if (kt + 1 < nk) store_tile(cur ^ 1);
      __syncthreads();
    }
  };

  load_group(0);
  load_tile(0);
  store_tile(0);
  __syncthreads();
  int ks = 0;
  for (int jg = 0; jg < G; ++jg) {
    begin(jg);
    for (int t = 0; t < spg; ++t, ++ks) kstep(ks);
    drain();
  }

  // C/D layout (gfx950, dtype independent): col = lane & 31, row = (r&3) + 8*(r>>2) + 4*(lane>>5)
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int64_t gm = m0 + wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
        if (gm < M && gcol[j] < N) C[gm * ldc + gcol[j]] = (float)facc[i][j][r];
      }
    }
#undef AS
#undef BS
}

// gsum[j][n] = sum_{k in group j} bt[n][k]: one thread per (j, n), 16 bytes per load
__global__ void __launch_bounds__(256)
k_group_colsum(const int8_t* __restrict__ bt, int64_t N, int64_t ldb, int64_t g, int64_t G, int32_t* __restrict__ gsum) {
  const int64_t total = G * N, stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const int64_t j = i / N, n = i - j * N;
    const v4i* p = reinterpret_cast<const v4i*>(bt + n * ldb + j * g);
    int s = 0;
    for (int64_t c = 0; c < g / 16; ++c) {
      const v4i v = p[c];
#pragma unroll
      for (int e = 0; e < 4; ++e) s = __builtin_amdgcn_sdot4(v[e], 0x01010101, s, false);
    }
    gsum[i] = s;
  }
}

}  // namespace
}  // namespace nqk

using namespace nqk;

// What both entries refuse.  0 to go on, -1 with the error recorded.
static int check_group(const std::string& who, const void* bt, int64_t N, int64_t K, int64_t ldb, int64_t g) {
  if (g < 32 || (g & 31)) return fail(who + ": the group size must be a positive multiple of 32");
  if (g > 16384) return fail(who + ": a group size above 16384 leaves f64(sg) * f64(P_j) inexact");
  if (K <= 0 || K % g) return fail(who + ": K must be a positive multiple of the group size");
  if (N <= 0) return fail(who + ": N must be positive");
  if ((ldb & 15) || ldb < K) return fail(who + ": ldb must be a multiple of 16 and at least K");
  if (!bt || (((uintptr_t)bt) & 15)) return fail(who + ": bt must be a 16-byte aligned pointer");
  return 0;
}

extern "C" int nqk_group_colsum(const int8_t* bt, int64_t N, int64_t K, int64_t ldb, int64_t g, int32_t* gsum) {
  const char* who = "nqk_group_colsum";
  if (check_group(who, bt, N, K, ldb, g)) return -1;
  if (!gsum || (((uintptr_t)gsum) & 3)) return fail("nqk_group_colsum: gsum must be a 4-byte aligned pointer");
  const int64_t G = K / g;
  hipLaunchKernelGGL(k_group_colsum, dim3(grid_for(G * N)), dim3(kThreads), 0, stream(), bt, N, ldb, g, G, gsum);
  return launch_status(who);
}

extern "C" int nqk_qgemm_group(const int8_t* a, const int8_t* bt, const float* sg, const int32_t* gsum, float* out,
                               int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldb, int64_t ldo, int64_t g,
                               int64_t zpa, int has_zpa) {
  const std::string who = "nqk_qgemm_group";
  if (check_group(who, bt, N, K, ldb, g)) return -1;
  if (M <= 0) return 0;
  if ((lda & 15) || lda < K) return fail(who + ": lda must be a multiple of 16 and at least K");
  if (ldo < N) return fail(who + ": ldo is shorter than a row of the output");
  if (!a || (((uintptr_t)a) & 15)) return fail(who + ": a must be a 16-byte aligned pointer");
  if (!sg || (((uintptr_t)sg) & 3) || !out || (((uintptr_t)out) & 3))
    return fail(who + ": sg and out must be 4-byte aligned pointers");
  if (has_zpa && (!gsum || (((uintptr_t)gsum) & 3)))
    return fail(who + ": a zero point needs gsum, a 4-byte aligned pointer (nqk_group_colsum)");
  if (has_zpa && (zpa < -128 || zpa > 127)) return fail(who + ": the zero point of an int8 activation lies in -128..127");
  const int64_t tiles_m = (M + BM - 1) / BM, tiles_n = (N + BN - 1) / BN;
  if (tiles_m * tiles_n > 0x7fffffff) return fail(who + ": too many tiles");
  hipLaunchKernelGGL(k_qgemm_group, dim3((unsigned)(tiles_m * tiles_n)), dim3(256), 0, stream(), a, bt, sg,
                     has_zpa ? gsum : nullptr, out, M, N, K, lda, ldb, ldo, (int)(g / 32), (int)(K / g),
                     has_zpa ? (int)zpa : 0, (int)tiles_n);
  return launch_status(who.c_str());
}
