// OCP Microscaling operands (Model.quantize(mx_format=...)): the block quantizer and the GEMM on
// CDNA4's block-scaled matrix instruction v_mfma_scale_f32_32x32x64_f8f6f4.
//
// Format (include/nqk.h states it; tests/_mx_ref.py is its NumPy restatement).  A block is 32
// consecutive k of one row.  amax = max |v|; e = max(exponent(amax) - emax_elem, -127), taken from
// amax's float32 exponent field (a subnormal amax gives -127, an all-zero block e = 0); the scale byte
// is e + 127 (E8M0); element = round_to_format(v * 2^-e), nearest with ties to even, saturating.
// fp8 is E4M3 (bias 7, largest 448, emax_elem 8), one byte per element; fp4 is E2M1 (largest 6,
// emax_elem 2), two per byte, even k in the low nibble.
//
// nqk_quantize_mx reads x once.  A lane owns a float4, so 8 consecutive lanes own a block and a wave
// owns 256 columns of one stored row; the chunks of the K padding (cols .. ldq - 1) are lanes like any
// other that load nothing, so they store zero elements and the scale byte 127.  |v| as an integer
// orders like the float, so amax is an unsigned max over the lane's four values and three lane
// exchanges (xor 1, 2, 4).  2^-e is built in the exponent field (127 - e lies in 2..254: a normal
// float), the product v * 2^-e is exact unless it underflows, far below half the smallest subnormal
// of either format, and the code is cut out of the product's bits with integer arithmetic: add
// half an ulp of the target mantissa minus one plus the kept mantissa's last bit, shift, clamp.  Below
// the format's smallest normal the code is rint(|t| / quantum).  fp8: a dword of 4 codes per lane;
// fp4: a lane's 4 nibbles and its neighbour's make the dword the even lane stores.  No LDS.
//
// nqk_gemm_mx: 128 x 128 output tile, 4 waves (2 x 2, 64 x 64 each = 2 x 2 tiles of the 32 x 32 x 64
// instruction, 64 float accumulators per lane), k-step 128.  Operand tiles go global -> registers ->
// LDS, double-buffered: a row of a tile is 128 bytes at fp8 (8 chunks of 16) and 64 at fp4 (4
// chunks).  In the instruction lane l supplies row (column) l % 32 and, with h = l / 32, at fp4 the 32
// consecutive k from 32 h (16 bytes), at fp8 the 16 k from 16 h in registers 0-3 and the 16 k from
// 32 + 16 h in registers 4-7 (measured: the first reading, 32 consecutive bytes, summed k 16..31 into
// block 1).  The lane's scale byte belongs to (row l % 32, block h) at either width, whichever lanes
// hold that block's elements.  The
// lanes of one ds_read_b128 pass are 16 consecutive rows at one chunk column, so chunk c of row r is
// stored at c ^ ((r >> 1) & 7) (128-byte rows) or c ^ ((r >> 2) & 3) (64-byte rows): 16 distinct
// 16-byte bank slots.  Scale bytes do not pass through LDS: the four bytes of a row's k-step are one
// aligned dword (the scale pitch is ld / 32, ld a multiple of 128), which the lane that owns the row
// loads a k-step ahead; shifted right by 8 for the upper half-wave, bytes 0 and 2 are the lane's own
// blocks of the two 64-wide sub-steps, selected by the instruction's op_sel.  M and N edges are
// guarded; K is not: the operands are zero elements with finite scales from K to the next multiple
// of 128, as nqk_quantize_mx stores them.
#include "nqk_common.h"

namespace nqk {
namespace {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v8i __attribute__((ext_vector_type(8)));
typedef float v16f __attribute__((ext_vector_type(16)));

// ------------------------------------------------------------------------------- block quantizer
// E4M3 code of t, |t| < 512 (finite): sign | 4 exponent bits (bias 7) | 3 mantissa bits
__device__ __forceinline__ uint32_t code_e4m3(float t) {
  const uint32_t u = __float_as_uint(t), a = u & 0x7fffffffu;
  uint32_t r;
  if (a >= (121u << 23)) {  // 2^-6, the smallest normal
    const uint32_t c = a - (120u << 23);
    r = (c + 0x7ffffu + ((c >> 20) & 1u)) >> 20;
    r = r > 0x7eu ? 0x7eu : r;
  } else {
    r = (uint32_t)(int)__builtin_rintf(__uint_as_float(a) * 512.0f);  // quantum 2^-9; 8 is 2^-6
  }
  return r | ((u >> 24) & 0x80u);
}

// E2M1 code of t, |t| < 8: sign | 2 exponent bits (bias 1) | 1 mantissa bit
__device__ __forceinline__ uint32_t code_e2m1(float t) {
  const uint32_t u = __float_as_uint(t), a = u & 0x7fffffffu;
  uint32_t r;
  if (a >= (127u << 23)) {  // 1, the smallest normal
    const uint32_t c = a - (126u << 23);
    r = (c + 0x1fffffu + ((c >> 22) & 1u)) >> 22;
    r = r > 7u ? 7u : r;
  } else {
    r = (uint32_t)(int)__builtin_rintf(__uint_as_float(a) * 2.0f);  // quantum 0.5; 2 is 1.0
  }
  return r | ((u >> 28) & 8u);
}

template <bool FP4>
__global__ void __launch_bounds__(256)
k_quantize_mx(const float* __restrict__ x, uint8_t* __restrict__ q, uint8_t* __restrict__ sc, int64_t rows,
              int64_t cols, int64_t ldx, int64_t ldq) {
  constexpr int EMAX = FP4 ? 2 : 8;
  const int64_t cpr = ldq >> 2;  // float4 chunks of a stored row, a multiple of 8
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool live = g < rows * cpr;  // whole groups of 8 lanes are live or not
  const int64_t row = live ? g / cpr : 0, c = live ? g % cpr : 0;
  const int64_t k = 4 * c;
  float4 v = {0.0f, 0.0f, 0.0f, 0.0f};
  if (live && k < cols) {  // cols is a multiple of 32: a chunk lies inside it or in the padding
    const float* p = x + row * ldx + k;
    if ((((uintptr_t)p) & 15) == 0) v = *reinterpret_cast<const float4*>(p);
    else v = float4{p[0], p[1], p[2], p[3]};
  }
  const uint32_t m = 0x7fffffffu;
  uint32_t am = max(max(__float_as_uint(v.x) & m, __float_as_uint(v.y) & m),
                    max(__float_as_uint(v.z) & m, __float_as_uint(v.w) & m));
  am = max(am, (uint32_t)__shfl_xor((int)am, 1, 64));
  am = max(am, (uint32_t)__shfl_xor((int)am, 2, 64));
  am = max(am, (uint32_t)__shfl_xor((int)am, 4, 64));
  const int e = am ? max((int)(am >> 23) - 127 - EMAX, -127) : 0;
  const float inv = __uint_as_float((uint32_t)(127 - e) << 23);  // 2^-e
  if (FP4) {
    const uint32_t h = code_e2m1(v.x * inv) | (code_e2m1(v.y * inv) << 4) | (code_e2m1(v.z * inv) << 8) |
                       (code_e2m1(v.w * inv) << 12);
    const uint32_t o = (uint32_t)__shfl_xor((int)h, 1, 64);
    if (live && !(c & 1)) *reinterpret_cast<uint32_t*>(q + row * (ldq >> 1) + 2 * c) = h | (o << 16);
  } else {
    const uint32_t w = code_e4m3(v.x * inv) | (code_e4m3(v.y * inv) << 8) | (code_e4m3(v.z * inv) << 16) |
                       (code_e4m3(v.w * inv) << 24);
    if (live) *reinterpret_cast<uint32_t*>(q + row * ldq + 4 * c) = w;
  }
  if (live && !(c & 7)) sc[row * (ldq >> 5) + (c >> 3)] = (uint8_t)(e + 127);
}

// ------------------------------------------------------------------------------- block-scaled GEMM
constexpr int BM = 128, BN = 128;  // the k-step is 128 elements: 16 * P bytes of a row, P = 8 (fp8) or 4 (fp4)

template <int P>
__device__ __forceinline__ int mx_swz(int row, int chunk) {
  return row * (16 * P) + ((chunk ^ ((row / (16 / P)) & (P - 1))) << 4);
}

// the lane's 32 values of `row` in sub-step s.  fp4: one chunk, the 32 consecutive k from 32 half (upper
// registers unused).  fp8: registers 0-3 are the 16 k from 16 half and registers 4-7 the 16 k from
// 32 + 16 half, so chunks half and 2 + half of the sub-step's four
template <int P>
__device__ __forceinline__ v8i mx_fragment(const uint8_t* tile, int row, int s, int half) {
  if (P == 8) {
    const v4i lo = *reinterpret_cast<const v4i*>(tile + mx_swz<P>(row, 4 * s + half));
    const v4i hi = *reinterpret_cast<const v4i*>(tile + mx_swz<P>(row, 4 * s + 2 + half));
    return v8i{lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
  }
  const v4i lo = *reinterpret_cast<const v4i*>(tile + mx_swz<P>(row, 2 * s + half));
  return v8i{lo.x, lo.y, lo.z, lo.w, 0, 0, 0, 0};
}

template <int PA, int PB>
__global__ void __launch_bounds__(256)
k_gemm_mx(const uint8_t* __restrict__ A, const uint8_t* __restrict__ As, const uint8_t* __restrict__ Bt,
          const uint8_t* __restrict__ Bs, float* __restrict__ C, int64_t M, int64_t N, int nk, int64_t lda,
          int64_t ldb, int64_t sa, int64_t sb, int64_t ldc, int tiles_n) {
  // lda, ldb: bytes of a row; sa, sb: scale bytes of a row
  constexpr int TA = BM * 16 * PA, TB = BN * 16 * PB;
  constexpr int FA = PA == 8 ? 0 : 4, FB = PB == 8 ? 0 : 4;  // cbsz / blgp: 0 = E4M3, 4 = E2M1
  __shared__ __attribute__((aligned(16))) uint8_t smem[2 * (TA + TB)];
#define AS(buf) (smem + (buf) * (TA + TB))
#define BS(buf) (smem + (buf) * (TA + TB) + TA)

  const int tm = blockIdx.x / tiles_n, tn = blockIdx.x % tiles_n;
  const int64_t m0 = (int64_t)tm * BM, n0 = (int64_t)tn * BN;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int r32 = lane & 31, half = lane >> 5;

  v4i ra[PA / 2], rb[PB / 2];  // 128 * P chunks of a tile over 256 threads
  auto load_tile = [&](int kt) {
    const v4i zero = {0, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < PA / 2; ++i) {
      const int idx = tid + i * 256, row = idx / PA, ch = idx % PA;
      const int64_t gm = m0 + row;
      ra[i] = gm < M ? *reinterpret_cast<const v4i*>(A + gm * lda + (int64_t)kt * (16 * PA) + ch * 16) : zero;
    }
#pragma unroll
    for (int i = 0; i < PB / 2; ++i) {
      const int idx = tid + i * 256, row = idx / PB, ch = idx % PB;
      const int64_t gn = n0 + row;
      rb[i] = gn < N ? *reinterpret_cast<const v4i*>(Bt + gn * ldb + (int64_t)kt * (16 * PB) + ch * 16) : zero;
    }
  };
  auto store_tile = [&](int buf) {
#pragma unroll
    for (int i = 0; i < PA / 2; ++i) {
      const int idx = tid + i * 256;
      *reinterpret_cast<v4i*>(AS(buf) + mx_swz<PA>(idx / PA, idx % PA)) = ra[i];
    }
#pragma unroll
    for (int i = 0; i < PB / 2; ++i) {
      const int idx = tid + i * 256;
      *reinterpret_cast<v4i*>(BS(buf) + mx_swz<PB>(idx / PB, idx % PB)) = rb[i];
    }
  };

  // the lane's rows and columns, and the scale dword (4 blocks of a k-step) of each; 2^0 past the edge
  int64_t grow[2], gcol[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    grow[i] = m0 + wm * 64 + i * 32 + r32;
    gcol[i] = n0 + wn * 64 + i * 32 + r32;
  }
  auto load_scales = [&](int kt, uint32_t (&xa)[2], uint32_t (&xb)[2]) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      xa[i] = grow[i] < M ? *reinterpret_cast<const uint32_t*>(As + grow[i] * sa + 4 * (int64_t)kt) : 0x7f7f7f7fu;
      xb[i] = gcol[i] < N ? *reinterpret_cast<const uint32_t*>(Bs + gcol[i] * sb + 4 * (int64_t)kt) : 0x7f7f7f7fu;
    }
  };

  v16f acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

  uint32_t xa[2], xb[2], na[2], nb[2];
  load_tile(0);
  load_scales(0, xa, xb);
  store_tile(0);
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const int cur = kt & 1;
    const bool last = kt + 1 == nk;
    if (!last) {
      load_tile(kt + 1);
      load_scales(kt + 1, na, nb);
    }
    int ea[2], eb[2];  // byte 0: the lane's block of sub-step 0, byte 2: of sub-step 1
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      ea[i] = (int)(xa[i] >> (8 * half));
      eb[i] = (int)(xb[i] >> (8 * half));
    }
    v8i fa[2], fb[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) fa[i] = mx_fragment<PA>(AS(cur), wm * 64 + i * 32 + r32, 0, half);
#pragma unroll
    for (int j = 0; j < 2; ++j) fb[j] = mx_fragment<PB>(BS(cur), wn * 64 + j * 32 + r32, 0, half);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(fa[i], fb[j], acc[i][j], FA, FB, 0, ea[i], 0, eb[j]);
#pragma unroll
    for (int i = 0; i < 2; ++i) fa[i] = mx_fragment<PA>(AS(cur), wm * 64 + i * 32 + r32, 1, half);
#pragma unroll
    for (int j = 0; j < 2; ++j) fb[j] = mx_fragment<PB>(BS(cur), wn * 64 + j * 32 + r32, 1, half);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(fa[i], fb[j], acc[i][j], FA, FB, 2, ea[i], 2, eb[j]);
    if (!last) {
      store_tile(cur ^ 1);
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        xa[i] = na[i];
        xb[i] = nb[i];
      }
    }
    __syncthreads();
  }

  // C/D layout (gfx950, dtype independent): col = lane & 31, row = (r&3) + 8*(r>>2) + 4*(lane>>5)
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int64_t gm = m0 + wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
#pragma unroll
      for (int j = 0; j < 2; ++j)
        if (gm < M && gcol[j] < N) C[gm * ldc + gcol[j]] = acc[i][j][r];
    }
#undef AS
#undef BS
}

}  // namespace
}  // namespace nqk

using namespace nqk;

static bool misaligned(const void* p, uintptr_t a) { return !p || (((uintptr_t)p) & (a - 1)); }
static bool mx_format(int f) { return f == NQK_MXFP8 || f == NQK_MXFP4; }

extern "C" int nqk_quantize_mx(const float* x, uint8_t* q, uint8_t* scales, int64_t rows, int64_t cols, int64_t ldx,
                               int64_t ldq, int format) {
  const std::string who = "nqk_quantize_mx";
  if (!mx_format(format)) return fail(who + ": format must be NQK_MXFP8 or NQK_MXFP4");
  if (rows < 0 || cols <= 0 || (cols & 31)) return fail(who + ": rows must not be negative and cols must be a positive multiple of 32");
  if (ldx < cols) return fail(who + ": ldx is shorter than a row");
  if (ldq < cols || (ldq & 31)) return fail(who + ": ldq must be a multiple of 32 and at least cols");
  if (misaligned(x, 4) || misaligned(q, 4)) return fail(who + ": x and q must be 4-byte aligned pointers");
  if (!scales) return fail(who + ": scales must not be NULL");
  if (rows == 0) return 0;
  const int64_t blocks = (rows * (ldq >> 2) + 255) / 256;
  if (rows > 0x7fffffff || blocks > 0x7fffffff) return fail(who + ": too many blocks");
  if (format == NQK_MXFP4)
    hipLaunchKernelGGL(k_quantize_mx<true>, dim3((unsigned)blocks), dim3(256), 0, stream(), x, q, scales, rows, cols, ldx, ldq);
  else
    hipLaunchKernelGGL(k_quantize_mx<false>, dim3((unsigned)blocks), dim3(256), 0, stream(), x, q, scales, rows, cols, ldx, ldq);
  return launch_status(who.c_str());
}

extern "C" int nqk_gemm_mx(const uint8_t* a, const uint8_t* a_scales, int a_format, const uint8_t* bt,
                           const uint8_t* b_scales, int b_format, float* out, int64_t M, int64_t N, int64_t K,
                           int64_t lda, int64_t ldb, int64_t ldo) {
  const std::string who = "nqk_gemm_mx";
  if (!mx_format(a_format) || !mx_format(b_format)) return fail(who + ": a format must be NQK_MXFP8 or NQK_MXFP4");
  if (a_format == NQK_MXFP4 && b_format == NQK_MXFP8) return fail(who + ": fp4 activations with fp8 weights are not built");
  if (K <= 0 || (K & 31)) return fail(who + ": K must be a positive multiple of 32");
  if (N <= 0) return fail(who + ": N must be positive");
  if ((ldb & 127) || ldb < K) return fail(who + ": ldb must be a multiple of 128 and at least K");
  if (misaligned(bt, 16)) return fail(who + ": bt must be a 16-byte aligned pointer");
  if (misaligned(b_scales, 4)) return fail(who + ": b_scales must be a 4-byte aligned pointer");
  if (M <= 0) return 0;
  if ((lda & 127) || lda < K) return fail(who + ": lda must be a multiple of 128 and at least K");
  if (ldo < N) return fail(who + ": ldo is shorter than a row of the output");
  if (misaligned(a, 16)) return fail(who + ": a must be a 16-byte aligned pointer");
  if (misaligned(a_scales, 4) || misaligned(out, 4)) return fail(who + ": a_scales and out must be 4-byte aligned pointers");
  const int64_t tiles_m = (M + BM - 1) / BM, tiles_n = (N + BN - 1) / BN;
  if (tiles_m * tiles_n > 0x7fffffff || K > 0x7fffffff) return fail(who + ": too many tiles");
  const int nk = (int)((K + 127) / 128);
  const dim3 grid((unsigned)(tiles_m * tiles_n)), block(256);
  const int64_t la = a_format == NQK_MXFP8 ? lda : lda >> 1, lb = b_format == NQK_MXFP8 ? ldb : ldb >> 1;
#define MX_LAUNCH(PA, PB)                                                                                          \
  hipLaunchKernelGGL((k_gemm_mx<PA, PB>), grid, block, 0, stream(), a, a_scales, bt, b_scales, out, M, N, nk, la, lb, \
                     lda >> 5, ldb >> 5, ldo, (int)tiles_n)
  if (a_format == NQK_MXFP8 && b_format == NQK_MXFP8) MX_LAUNCH(8, 8);
  else if (a_format == NQK_MXFP8) MX_LAUNCH(8, 4);
  else MX_LAUNCH(4, 4);
#undef MX_LAUNCH
  return launch_status(who.c_str());
}
