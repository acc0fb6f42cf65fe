// nqk_qgemm_i16 — q_matmul's integer product (numpy_quantization.py:47) for 9..16-bit
// activations (int16 storage) on the int8 MFMAs, exact, int64 out.
//
// Byte planes.  An int16 x is two bytes.  With xh = x >> 8 (the signed high byte) and
// xl = (x & 255) - 128 (the low byte with its top bit flipped) both planes are signed bytes
// and x = 256 xh + xl + 128.  (The symmetric split, a signed low byte and the rest in the
// high part, needs a high part of 128 for x >= 32640; the offset split has no such value.)
// With x' = 256 xh + xl = x - 128:
//   int16 x int8 :  sum a b = 256 sum ah b + sum al b + 128 sum_k b
//   int16 x int16:  sum a b = 65536 sum ah bh + 256 (sum ah bl + sum al bh) + sum al bl
//                             + 128 (sum_k a' + sum_k b') + 16384 Kp
// Kp is the length the MFMAs sum: K rounded up to the 64 of a k-step.  The tile is padded
// with int16 zeros BEFORE the split, so a padded position is a real zero operand
// (0 = 256 * 0 + (-128) + 128) and the identity holds over Kp positions as it stands.
//
// Frame: k_qgemm_i8's (nqk_gemm.hip).  128 x 128 x 64 tile, 4 waves (2 x 2, 64 x 64 each =
// 2 x 2 tiles of v_mfma_i32_32x32x32_i8), double-buffered LDS with its swizzle.  A thread
// stages the same (row, 16-k chunk) pairs as there; for an int16 operand it loads the 32
// bytes of the chunk once and splits them in registers (two v_perm_b32 and one v_xor per
// four values) into one 16-byte chunk of the high plane and one of the low plane.  LDS
// holds each plane as an int8 tile of k_qgemm_i8's layout, so the fragment reads are its
// reads.  One accumulator set per power of 256: two with an int8 B, three with an int16 B
// (the cross planes ah bl and al bh share one).  Every plane product is at most 2^14 and
// the shared accumulator holds at most 2^15 K, hence K < 2^16.
//
// The sums over k come from v_dot4_i32_i8 against 0x01010101 on the bytes a thread stages
// anyway: its rows are the same in every k-step, so it keeps one int32 per row and plane
// and the four threads of a row are added once, after the k loop, through LDS.  (The other
// way, an MFMA against an all-ones operand as k_attn_long does, costs a quarter or an
// eighth more MFMA work and an accumulator set of which one column is used; the staging
// VALU work here hides under the MFMAs.)  The planes meet in int64 once per tile.
//
// nqk_qgemm_i16_epi — the same main loop ending in the product's one consumer instead of the
// int64 store: nqk_dequantize(_cols) (f32 out) or nqk_requantize(_cols) (int16 out), in their
// arithmetic (nqk_requant.h).  int64 addition is exact in any order, so what depends on the
// column alone (128 sum_k b, 16384 Kp, bias[n], -col[n] zpa, +zpa zpb K) is folded into scol when
// it is written and what depends on the row alone (128 sum_k a', -row[m] zpb) into srow: an
// output adds two int64 terms to its planes, converts once to f64 and multiplies by its column's
// scale, which a lane loads once per column (it owns 2 columns x 32 rows).  Stores go straight
// from the C/D layout: one instruction covers 32 consecutive columns of 2 rows.
#include "nqk_common.h"
#include "nqk_requant.h"

namespace nqk {
namespace {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));

constexpr int BM = 128, BN = 128, BK = 64;
constexpr int PLANE = BM * BK;  // bytes of one int8 plane tile (BM == BN)

__device__ __forceinline__ int dot_ones(const v4i& c, int s) {
  s = __builtin_amdgcn_sdot4(c[0], 0x01010101, s, false);
  s = __builtin_amdgcn_sdot4(c[1], 0x01010101, s, false);
  s = __builtin_amdgcn_sdot4(c[2], 0x01010101, s, false);
  return __builtin_amdgcn_sdot4(c[3], 0x01010101, s, false);
}

// 16 int16 (two 16-byte loads) -> their high bytes and their offset low bytes, 16 each
__device__ __forceinline__ void split16(const v4i& x0, const v4i& x1, v4i& hi, v4i& lo) {
  hi[0] = (int)__builtin_amdgcn_perm((unsigned)x0[1], (unsigned)x0[0], 0x07050301u);
  hi[1] = (int)__builtin_amdgcn_perm((unsigned)x0[3], (unsigned)x0[2], 0x07050301u);
  hi[2] = (int)__builtin_amdgcn_perm((unsigned)x1[1], (unsigned)x1[0], 0x07050301u);
  hi[3] = (int)__builtin_amdgcn_perm((unsigned)x1[3], (unsigned)x1[2], 0x07050301u);
  lo[0] = (int)(__builtin_amdgcn_perm((unsigned)x0[1], (unsigned)x0[0], 0x06040200u) ^ 0x80808080u);
  lo[1] = (int)(__builtin_amdgcn_perm((unsigned)x0[3], (unsigned)x0[2], 0x06040200u) ^ 0x80808080u);
  lo[2] = (int)(__builtin_amdgcn_perm((unsigned)x1[1], (unsigned)x1[0], 0x06040200u) ^ 0x80808080u);
  lo[3] = (int)(__builtin_amdgcn_perm((unsigned)x1[3], (unsigned)x1[2], 0x06040200u) ^ 0x80808080u);
}

// What the fused epilogue needs beyond the product's own arguments (OUT != NQK_I64)
struct Epi16 {
  const float* s_col;  // [N] per-column scales, or null: `scale`
  double scale;
  int flags;           // NQK_ZP_ROW | COL | KCONST
  int64_t zpa, zpb, zK;
  const int64_t* row;
  const int64_t* col;
  const void* bias;    // [N] of bias_dtype, or null
  int bias_dtype;
  float res_scale;
  double rz;
  int has_rz;
  double lo, hi;
  float flo, fhi;
};

__device__ __forceinline__ int64_t load_int(const void* p, int dtype, int64_t i) {
  switch (dtype) {
    case NQK_I8: return reinterpret_cast<const int8_t*>(p)[i];
    case NQK_I16: return reinterpret_cast<const int16_t*>(p)[i];
    case NQK_I32: return reinterpret_cast<const int32_t*>(p)[i];
    default: return reinterpret_cast<const int64_t*>(p)[i];
  }
}

// WIDE: Bt is int16 (three accumulator sets), else int8 (two).  OUT: NQK_I64 stores the product
// (nqk_qgemm_i16); NQK_F32 dequantizes it and NQK_I16 requantizes it (nqk_qgemm_i16_epi, `e`).
template <bool WIDE, int OUT>
__global__ void __launch_bounds__(256)
k_qgemm_i16(const int16_t* __restrict__ A, const void* __restrict__ Btv, void* __restrict__ Cv, int64_t M, int64_t N,
            int64_t K, int64_t lda, int64_t ldb, int64_t ldc, BatchMap bm, int64_t a_ms, int64_t b_ms, int64_t c_ms,
            int tiles_n, Epi16 e) {
  constexpr bool EPI = OUT != NQK_I64;
  constexpr int NB = WIDE ? 2 : 1;          // planes of B
  constexpr int BUF = (2 + NB) * PLANE;     // one buffer: A high, A low, B (high, low | the bytes)
  __shared__ __attribute__((aligned(16))) int8_t smem[2 * BUF];
#define AH(buf) (smem + (buf) * BUF)
#define AL(buf) (smem + (buf) * BUF + PLANE)
#define BH(buf) (smem + (buf) * BUF + 2 * PLANE)
#define BL(buf) (smem + (buf) * BUF + 3 * PLANE)

  const int64_t bz = blockIdx.z;
  A += map_a(bm, bz) * a_ms;
  const int16_t* B16 = reinterpret_cast<const int16_t*>(Btv) + map_b(bm, bz) * b_ms;
  const int8_t* B8 = reinterpret_cast<const int8_t*>(Btv) + map_b(bm, bz) * b_ms;
  int64_t* C = reinterpret_cast<int64_t*>(Cv) + (EPI ? 0 : bz * c_ms);
  const int tm = blockIdx.x / tiles_n, tn = blockIdx.x % tiles_n;
  const int64_t m0 = (int64_t)tm * BM, n0 = (int64_t)tn * BN;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;

  // staging: 512 (row, 16-k chunk) pairs per operand tile, 2 per thread; an int16 pair is 32 bytes
  v4i ra[2][2], rb[2][NB];
  int sum_ah[2] = {0, 0}, sum_al[2] = {0, 0}, sum_bh[2] = {0, 0}, sum_bl[2] = {0, 0};
  auto load_tile = [&](int64_t k0) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int idx = tid + i * 256, row = idx >> 2, ch = idx & 3;
      const int64_t kk = k0 + ch * 16;  // K % 16 == 0: a chunk lies inside K or outside it
      const int64_t gm = m0 + row, gn = n0 + row;
      const v4i z = {0, 0, 0, 0};
      const bool oka = gm < M && kk < K, okb = gn < N && kk < K;
      const v4i* pa = reinterpret_cast<const v4i*>(A + gm * lda + kk);
      ra[i][0] = oka ? pa[0] : z;
      ra[i][1] = oka ? pa[1] : z;
      if constexpr (WIDE) {
        const v4i* pb = reinterpret_cast<const v4i*>(B16 + gn * ldb + kk);
        rb[i][0] = okb ? pb[0] : z;
        rb[i][1] = okb ? pb[1] : z;
      } else {
        rb[i][0] = okb ? *reinterpret_cast<const v4i*>(B8 + gn * ldb + kk) : z;
      }
    }
  };
  auto store_tile = [&](int buf) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int idx = tid + i * 256, off = swz(idx >> 2, idx & 3);
      v4i hi, lo;
      split16(ra[i][0], ra[i][1], hi, lo);
      *reinterpret_cast<v4i*>(AH(buf) + off) = hi;
      *reinterpret_cast<v4i*>(AL(buf) + off) = lo;
      if constexpr (WIDE) {
        sum_ah[i] = dot_ones(hi, sum_ah[i]);
        sum_al[i] = dot_ones(lo, sum_al[i]);
        split16(rb[i][0], rb[i][1], hi, lo);
        *reinterpret_cast<v4i*>(BH(buf) + off) = hi;
        *reinterpret_cast<v4i*>(BL(buf) + off) = lo;
        sum_bh[i] = dot_ones(hi, sum_bh[i]);
        sum_bl[i] = dot_ones(lo, sum_bl[i]);
      } else {
        *reinterpret_cast<v4i*>(BH(buf) + off) = rb[i][0];
        sum_bl[i] = dot_ones(rb[i][0], sum_bl[i]);
      }
    }
  };

  // acc[0]: ah bh (ah b), acc[1]: the cross planes (al b), acc[2]: al bl
  constexpr int NACC = WIDE ? 3 : 2;
  v16i acc[NACC][2][2];
#pragma unroll
  for (int p = 0; p < NACC; ++p)
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[p][i][j][r] = 0;

  const int nk = (int)((K + BK - 1) / BK);
  load_tile(0);
  store_tile(0);
  __syncthreads();
  const int r32 = lane & 31, half = lane >> 5;
  for (int kt = 0; kt < nk; ++kt) {
    const int cur = kt & 1;
    if (kt + 1 < nk) load_tile((int64_t)(kt + 1) * BK);
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      v4i fah[2], fal[2], fbh[2], fbl[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int off = swz(wm * 64 + i * 32 + r32, 2 * s + half);
        fah[i] = *reinterpret_cast<const v4i*>(AH(cur) + off);
        fal[i] = *reinterpret_cast<const v4i*>(AL(cur) + off);
      }
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int off = swz(wn * 64 + j * 32 + r32, 2 * s + half);
        fbh[j] = *reinterpret_cast<const v4i*>(BH(cur) + off);
        if constexpr (WIDE) fbl[j] = *reinterpret_cast<const v4i*>(BL(cur) + off);
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          acc[0][i][j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(fah[i], fbh[j], acc[0][i][j], 0, 0, 0);
          acc[1][i][j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(fal[i], fbh[j], acc[1][i][j], 0, 0, 0);
          if constexpr (WIDE) {
            acc[1][i][j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(fah[i], fbl[j], acc[1][i][j], 0, 0, 0);
            acc[2][i][j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(fal[i], fbl[j], acc[2][i][j], 0, 0, 0);
          }
        }
    }
    if (kt + 1 < nk) store_tile(cur ^ 1);
    __syncthreads();
  }

  // the sums over k: the four threads of a row (adjacent lanes) are added, lane ch == 0 of
  // each row writes x' = 256 xh + xl summed (WIDE) or sum b (narrow) to LDS.  The barrier that
  // ended the k loop has retired every fragment read, so the tiles' space is free.
  // With an epilogue they also take what else depends on the row or on the column alone.
  int64_t* srow = reinterpret_cast<int64_t*>(smem);  // [BM]: 128 sum_k a'  (WIDE or EPI only)
  int64_t* scol = srow + BM;                         // [BN]: 128 (sum_k b' | sum_k b)
  const int64_t kconst = WIDE ? (int64_t)16384 * nk * BK : 0;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    int ah = sum_ah[i], al = sum_al[i], bh = sum_bh[i], bl = sum_bl[i];
#pragma unroll
    for (int d = 1; d < 4; d <<= 1) {
      bl += __shfl_xor(bl, d);
      if constexpr (WIDE) {
        ah += __shfl_xor(ah, d);
        al += __shfl_xor(al, d);
        bh += __shfl_xor(bh, d);
      }
    }
    if ((tid & 3) == 0) {
      const int row = (tid >> 2) + 64 * i;
      if constexpr (EPI) {
        const int64_t gm = m0 + row, gn = n0 + row;
        int64_t c = 128 * (256 * (int64_t)bh + bl) + kconst;
        int64_t r = WIDE ? 128 * (256 * (int64_t)ah + al) : 0;
        if (gn < N) {
          if (e.bias) c += load_int(e.bias, e.bias_dtype, gn);
          if (e.flags & NQK_ZP_COL) c -= e.col[map_b(bm, bz) * N + gn] * e.zpa;
        }
        if (e.flags & NQK_ZP_KCONST) c += e.zpa * e.zpb * e.zK;
        if ((e.flags & NQK_ZP_ROW) && gm < M) r -= e.row[map_a(bm, bz) * M + gm] * e.zpb;
        scol[row] = c;
        srow[row] = r;
      } else {
        scol[row] = 128 * (256 * (int64_t)bh + bl);
        if constexpr (WIDE) srow[row] = 128 * (256 * (int64_t)ah + al);
      }
    }
  }
  __syncthreads();

  if constexpr (EPI) {
    // acc64 (+ bias) - zp_term is planes + srow + scol; then the consumer's arithmetic per output
    float* of = reinterpret_cast<float*>(Cv) + bz * c_ms;
    int16_t* oq = reinterpret_cast<int16_t*>(Cv) + bz * c_ms;
    const float rr = 1.0f / e.res_scale;  // Python `1 / res_scale` on a float32 scalar
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int ln = wn * 64 + j * 32 + r32;
        const int64_t gn = n0 + ln;
        const int64_t cterm = scol[ln];
        const double s = e.s_col ? (gn < N ? (double)e.s_col[gn] : 0.0) : e.scale;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int lm = wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
          const int64_t gm = m0 + lm;
          int64_t v;
          if constexpr (WIDE)
            v = 65536 * (int64_t)acc[0][i][j][r] + 256 * (int64_t)acc[1][i][j][r] + (int64_t)acc[2][i][j][r];
          else
            v = 256 * (int64_t)acc[0][i][j][r] + (int64_t)acc[1][i][j][r];
          v += srow[lm] + cterm;
          const float d = (float)((double)v * s);
          if (gm < M && gn < N) {
            if constexpr (OUT == NQK_F32)
              of[gm * ldc + gn] = d;
            else
              oq[gm * ldc + gn] = (int16_t)requant_tail(d, rr, e.rz, e.has_rz, e.lo, e.hi, e.flo, e.fhi);
          }
        }
      }
    return;
  }

  // C/D layout (gfx950, dtype independent): col = lane & 31, row = (r&3) + 8*(r>>2) + 4*(lane>>5)
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int ln = wn * 64 + j * 32 + r32;
      const int64_t gn = n0 + ln;
      const int64_t cterm = scol[ln] + kconst;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int lm = wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
        const int64_t gm = m0 + lm;
        int64_t v;
        if constexpr (WIDE)
          v = 65536 * (int64_t)acc[0][i][j][r] + 256 * (int64_t)acc[1][i][j][r] + (int64_t)acc[2][i][j][r] + srow[lm] + cterm;
        else
          v = 256 * (int64_t)acc[0][i][j][r] + (int64_t)acc[1][i][j][r] + cterm;
        if (gm < M && gn < N) C[gm * ldc + gn] = v;
      }
    }
#undef AH
#undef AL
#undef BH
#undef BL
}

}  // namespace
}  // namespace nqk

using namespace nqk;

// What both entries refuse before a launch.  Returns 0 to go on, 1 when there is nothing to compute,
// -1 with the error recorded.  `omask`: the alignment of the output pointer.
static int check_operands(const std::string& who, const void* a, const void* bt, int bt_dtype, const void* out,
                          uintptr_t omask, int64_t batch, int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldb,
                          int64_t ldo, int64_t a_mat_stride, int64_t b_mat_stride) {
  if (bt_dtype != NQK_I8 && bt_dtype != NQK_I16) return fail(who + ": bt_dtype must be NQK_I8 or NQK_I16");
  if (batch <= 0 || M <= 0 || N <= 0) return 1;
  if (!a || !bt || !out) return fail(who + ": null operand");
  if (K <= 0 || (lda & 15) || (ldb & 15) || (K & 15)) return fail(who + ": lda, ldb and K must be positive multiples of 16");
  if (lda < K || ldb < K || ldo < N) return fail(who + ": a leading dimension is shorter than its row");
  // a matrix stride in elements: 16 bytes are 8 int16 or 16 int8
  const int64_t bmask = bt_dtype == NQK_I16 ? 7 : 15;
  if ((((uintptr_t)a) & 15) || (((uintptr_t)bt) & 15) || (((uintptr_t)out) & omask) || (a_mat_stride & 7) || (b_mat_stride & bmask))
    return fail(who + ": operands must be 16-byte aligned (the output: its element size)");
  if (batch > 65535) return fail(who + ": batch > 65535");
  // the shared cross accumulator holds up to 2^15 per product: 2^16 of them reach 2^31
  if (K >= (1 << 16)) return fail(who + ": K of 65536 or more can overflow the int32 accumulators (use nqk_qgemm_generic)");
  const int64_t tiles_m = (M + BM - 1) / BM, tiles_n = (N + BN - 1) / BN;
  if (tiles_m * tiles_n > 0x7fffffff) return fail(who + ": too many tiles");
  return 0;
}

template <int OUT>
static void launch16(bool wide, const int16_t* a, const void* bt, void* out, int64_t batch, int64_t M, int64_t N,
                     int64_t K, int64_t lda, int64_t ldb, int64_t ldo, const int64_t* bmap, int64_t a_ms, int64_t b_ms,
                     int64_t o_ms, const Epi16& e) {
  const int64_t tiles_m = (M + BM - 1) / BM, tiles_n = (N + BN - 1) / BN;
  const BatchMap m = batch_map(bmap);
  const dim3 grid((unsigned)(tiles_m * tiles_n), 1, (unsigned)batch);
  if (wide)
    hipLaunchKernelGGL((k_qgemm_i16<true, OUT>), grid, dim3(256), 0, stream(), a, bt, out, M, N, K, lda, ldb, ldo, m,
                       a_ms, b_ms, o_ms, (int)tiles_n, e);
  else
    hipLaunchKernelGGL((k_qgemm_i16<false, OUT>), grid, dim3(256), 0, stream(), a, bt, out, M, N, K, lda, ldb, ldo, m,
                       a_ms, b_ms, o_ms, (int)tiles_n, e);
}

extern "C" int nqk_qgemm_i16(const int16_t* a, const void* bt, int bt_dtype, int64_t* c, int64_t batch, int64_t M,
                             int64_t N, int64_t K, int64_t lda, int64_t ldb, int64_t ldc, const int64_t* bmap,
                             int64_t a_mat_stride, int64_t b_mat_stride, int64_t c_mat_stride) {
  const int rc = check_operands("nqk_qgemm_i16", a, bt, bt_dtype, c, 7, batch, M, N, K, lda, ldb, ldc, a_mat_stride,
                                b_mat_stride);
  if (rc) return rc < 0 ? rc : 0;
  launch16<NQK_I64>(bt_dtype == NQK_I16, a, bt, c, batch, M, N, K, lda, ldb, ldc, bmap, a_mat_stride, b_mat_stride,
                    c_mat_stride, Epi16{});
  return launch_status("nqk_qgemm_i16");
}

extern "C" int nqk_qgemm_i16_epi(const int16_t* a, const void* bt, int bt_dtype, void* out, int out_dtype,
                                 int64_t batch, int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldb, int64_t ldo,
                                 const int64_t* bmap, int64_t a_mat_stride, int64_t b_mat_stride,
                                 int64_t out_mat_stride, const nqk_gemm16_epilogue* p) {
  const char* who = "nqk_qgemm_i16_epi";
  if (!p) return fail("nqk_qgemm_i16_epi: null parameters");
  if (out_dtype != NQK_F32 && out_dtype != NQK_I16) return fail("nqk_qgemm_i16_epi: out_dtype must be NQK_F32 or NQK_I16");
  const bool requant = out_dtype == NQK_I16;
  if (requant && (p->bit_width < 9 || p->bit_width > 16))
    return fail("nqk_qgemm_i16_epi: bit_width of the int16 result must be 9..16");
  if (!requant && p->bias) return fail("nqk_qgemm_i16_epi: a bias belongs to the requantize form (out_dtype NQK_I16)");
  if (p->bias && (p->bias_dtype < NQK_I8 || p->bias_dtype > NQK_I64))
    return fail("nqk_qgemm_i16_epi: bias_dtype must be an integer dtype code");
  if (p->zp_flags & ~(NQK_ZP_ROW | NQK_ZP_COL | NQK_ZP_KCONST))
    return fail("nqk_qgemm_i16_epi: zp_flags other than ROW, COL and KCONST (SCALAR and FULL belong to no product)");
  if (((p->zp_flags & NQK_ZP_ROW) && !p->row) || ((p->zp_flags & NQK_ZP_COL) && !p->col))
    return fail("nqk_qgemm_i16_epi: a zp flag whose vector is null");
  const int rc = check_operands(who, a, bt, bt_dtype, out, requant ? 1 : 3, batch, M, N, K, lda, ldb, ldo,
                                a_mat_stride, b_mat_stride);
  if (rc) return rc < 0 ? rc : 0;
  Epi16 e;
  e.s_col = p->s_col; e.scale = (double)p->scale;
  e.flags = p->zp_flags; e.zpa = p->zpa; e.zpb = p->zpb; e.zK = p->zp_K; e.row = p->row; e.col = p->col;
  e.bias = p->bias; e.bias_dtype = p->bias_dtype;
  const QuantP q = make_qp(1.0f, 0, 0, requant ? p->bit_width : 16);
  e.res_scale = requant ? p->res_scale : 1.0f; e.rz = (double)p->res_zp; e.has_rz = p->has_res_zp;
  e.lo = q.lo; e.hi = q.hi; e.flo = q.flo; e.fhi = q.fhi;
  if (requant)
    launch16<NQK_I16>(bt_dtype == NQK_I16, a, bt, out, batch, M, N, K, lda, ldb, ldo, bmap, a_mat_stride, b_mat_stride,
                      out_mat_stride, e);
  else
    launch16<NQK_F32>(bt_dtype == NQK_I16, a, bt, out, batch, M, N, K, lda, ldb, ldo, bmap, a_mat_stride, b_mat_stride,
                      out_mat_stride, e);
  return launch_status(who);
}
