// nqk_qconv.hip — the Conv in integers (opt-in, QModel.integer_conv): the reference's own q_matmul
// (numpy_quantization.py:44-61) applied to the reference's own im2col (numpy_helper.py:18-70) of the
// QUANTIZED input, instead of the float Conv on the dequantized operands (model.py:95-100,
// tensor.py:328-336).  An integer sum has no order to reproduce: any tiling gives the same bits.
//
//  * nqk_im2col_q   — the integer twin of nqk_im2col: cols[(b, oy, ox)][(ki, kj, ci)] in the storage
//                     dtype of the input, padded cells = the zero point (it dequantizes to exactly
//                     0.0, what the float Conv pads with), optional int64 row sums (the zero-point
//                     term of a weight with a zero point).
//  * nqk_embed_qi8  — the ViT patch embedding of an int8 image on v_mfma_i32_16x16x64_i8, with the
//                     epilogue of nqk_embed_q (bias, class-token row, position embedding).
#include "nqk_common.h"

namespace nqk {
namespace {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef float v4f __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------------------------------
// One wave per patch row: lanes stride over the K = kh kw c columns, so the row sum is one wave
// reduction.  Every read is guarded by the bounds of its own cell; rows * kcols outputs.
template <typename T>
__global__ void k_im2col_q(const T* __restrict__ x, T* __restrict__ cols, int64_t* __restrict__ rowsum, int64_t n,
                           int64_t c, int64_t h, int64_t w, int64_t kh, int64_t kw, int64_t ph0, int64_t pw0,
                           int64_t sh, int64_t sw, int64_t ho, int64_t wo, int64_t pad) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  const int64_t kcols = kh * kw * c, rows = n * ho * wo;
  for (int64_t r = wave; r < rows; r += nwaves) {
    const int64_t ox = r % wo, t2 = r / wo, oy = t2 % ho, b = t2 / ho;
    int64_t s = 0;
    for (int64_t col = lane; col < kcols; col += 64) {
      const int64_t ci = col % c, t = col / c, kj = t % kw, ki = t / kw;
      const int64_t iy = oy * sh + ki - ph0, ix = ox * sw + kj - pw0;
      int64_t v = pad;
      if (iy >= 0 && iy < h && ix >= 0 && ix < w) v = (int64_t)x[((b * c + ci) * h + iy) * w + ix];
      cols[r * kcols + col] = (T)v;
      s += v;
    }
    if (rowsum) {
      for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
      if (lane == 0) rowsum[r] = s;
    }
  }
}

// ---------------------------------------------------------------------------------------
// k_embed_qi8: out[b][1 + t][n] = (f32(f64(acc - colterm[n]) * f64(scale)) + bias[n]) + pos[1 + t][n],
// acc[m][n] = sum_k patch[m][k] * wt[n][k] in int32, K ordered (ci, ki, kj).
//
// With that K order and 16-wide kernel rows, the 16 k-bytes one lane feeds an MFMA are one
// contiguous, 16-byte-aligned run of an image row: lane l of a 64-deep k step (channel ci, kernel
// rows 4 kk .. 4 kk + 3) reads row 4 kk + (l >> 4) of patch (l & 15) — the 16 lanes of a group
// read 256 contiguous bytes when their patches sit side by side.  So the image goes HBM/L2 ->
// VGPRs with no im2col matrix and no LDS image, and the weights are Wq.reshape(N, K) as it lies.
// Only the weights are staged: one channel (BN rows x 256 B) per stage, loaded into registers
// under the previous stage's MFMAs; chunk c of LDS row r sits at c ^ (r & 15), so the 16 lanes of
// every ds_read_b128 lane group ({rows 0-3, 12-15 of k group g, rows 4-11 of g ^ 1} and its
// likes) touch 16 distinct 16-B slots.
//
// The products are computed transposed (weights as the MFMA's A operand, as k_pg does): lane l
// then holds, per 16 x 16 tile, patch (l & 15) and the 4 CONSECUTIVE outputs 4 (l >> 4) + r —
// one 16-byte store, four lanes per 64 contiguous bytes of an output row.
// Tile 128 patches x 64 WN outputs, 4 waves as 2 x 2, each 64 patches x 32 WN outputs.
// F32: the host proved |acc - colterm| < 2^24 from the operands, so f32(v) is exact and the one
// f32 product rounds the same exact value as the f64 product does; otherwise the f64 product.
template <int WN, bool F32>
__global__ void __launch_bounds__(256, 2)
k_embed_qi8(const int8_t* __restrict__ q, const int8_t* __restrict__ wt, const int32_t* __restrict__ colterm,
            const float* __restrict__ bias, const float* __restrict__ pos, float* __restrict__ out, int64_t M,
            int64_t N, int C, int64_t hw, int64_t wo, int64_t H, int64_t W, float scale, int xcd, int64_t tiles_n) {
  constexpr int BN = 64 * WN, NJ = 2 * WN, NP = BN / 16;
  __shared__ __attribute__((aligned(16))) int8_t sw_[BN * 256];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1, r16 = lane & 15, g = lane >> 4;
  // XCD-aware tile order (nqk_xcd.h): the column tiles of one row panel, which read the same image
  // rows, share an L2
  int64_t tile = blockIdx.x;
  if (xcd) tile = xcd_remap<int64_t>(tile, (int64_t)gridDim.x, (int64_t)xcd);
  const int64_t tm = tile / tiles_n, tn = tile - tm * tiles_n;
  const int64_t m0 = tm * 128 + wm * 64, n0 = tn * BN;
  const int64_t K = (int64_t)C * 256, cstride = H * W;

  // kernel row g of channel 0 of this lane's patch in each of the wave's 4 patch subtiles (rows
  // past M read the last patch: in bounds, never stored)
  const int8_t* pa[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    int64_t m = m0 + 16 * i + r16;
    m = m < M ? m : M - 1;
    const int64_t img = m / hw, pt = m - img * hw, oy = pt / wo, ox = pt - oy * wo;
    pa[i] = q + ((img * C) * H + oy * 16 + g) * W + ox * 16;
  }
  // weights: thread t moves 16-B chunk t & 15 of rows (t >> 4) + 16 p
  const int wr = tid >> 4, wc = tid & 15;
  const int8_t* wsrc = wt + (n0 + wr) * K + wc * 16;
  v4i wreg[NP];
  auto load_w = [&](int ci) {
#pragma unroll
    for (int p = 0; p < NP; ++p) wreg[p] = *reinterpret_cast<const v4i*>(wsrc + (int64_t)(16 * p) * K + ci * 256);
  };
  auto store_w = [&]() {
#pragma unroll
    for (int p = 0; p < NP; ++p)  // (wr + 16 p) & 15 == wr
      *reinterpret_cast<v4i*>(sw_ + (wr + 16 * p) * 256 + ((wc ^ wr) << 4)) = wreg[p];
  };
  const int8_t* bsrc = sw_ + (wn * 32 * WN + r16) * 256;

  v4i acc[4][NJ];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[i][j] = v4i{0, 0, 0, 0};

  // The patch rows of a whole stage (4 k steps x 4 subtiles) live in registers: each k step refills
  // its own rows for the NEXT stage right after its MFMAs, so an image load has a full stage of
  // MFMAs (of both waves of the SIMD) to arrive in; the next stage's weights are loaded at the head
  // of the stage and written to LDS at its end, with the 16 younger patch loads still in flight.
  // The scheduling fences keep every load where it is written: left alone, the compiler sinks all
  // 24 loads of a stage to the stage's end, where the next stage waits for them at once.  (With the
  // rows loaded one k step ahead instead, the loop waited on memory latency: 125 us at ViT-Base
  // B = 256 against 97 for this form.)
  v4i a[4][4];
  load_w(0);
  store_w();
#pragma unroll
  for (int kk = 0; kk < 4; ++kk)
#pragma unroll
    for (int i = 0; i < 4; ++i) a[kk][i] = *reinterpret_cast<const v4i*>(pa[i] + (int64_t)(4 * kk) * W);
  // (the compiler orders these 16 loads as it likes, and the loop's counted waits are the minimum over
  // both ways into the loop: a stage's first k step waits until 9 loads are left in flight instead
  // of 23.  Waiting for all 16 here, which gives the loop its own counts, measured the same:
  // 98.9 against 96.7 us on two boxes whose nqk_embed_q differed as little)
  for (int ci = 0; ci < C; ++ci) {
    __syncthreads();  // this stage's weights are in LDS
    const int cn = ci + 1 < C ? ci + 1 : ci;  // (the last stage loads its own operands again: no branch
    load_w(cn);                               //  around the loads)
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      v4i b[NJ];
#pragma unroll
      for (int j = 0; j < NJ; ++j)
        b[j] = *reinterpret_cast<const v4i*>(bsrc + 16 * j * 256 + (((4 * kk + g) ^ r16) << 4));
#pragma unroll
      for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int j = 0; j < NJ; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(b[j], a[kk][i], acc[i][j], 0, 0, 0);
        a[kk][i] = *reinterpret_cast<const v4i*>(pa[i] + (int64_t)cn * cstride + (int64_t)(4 * kk) * W);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    __syncthreads();  // every wave has read this stage's fragments
    store_w();
  }

  // epilogue: lane holds patch 16 i + r16 and outputs 16 j + 4 g .. + 3 of the wave tile
  const int64_t nb = n0 + wn * 32 * WN + 4 * g;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int64_t m = m0 + 16 * i + r16;
    if (m >= M) continue;
    const int64_t img = m / hw, t = m - img * hw;
    float* orow = out + (m + img + 1) * N;  // behind the image's class-token row
    const float* prow = pos + (1 + t) * N;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int64_t n = nb + 16 * j;
      const v4i ct = *reinterpret_cast<const v4i*>(colterm + n);
      const v4f bi = *reinterpret_cast<const v4f*>(bias + n);
      const v4f po = *reinterpret_cast<const v4f*>(prow + n);
      v4f o;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int v = acc[i][j][r] - ct[r];  // host-checked: no int32 overflow
        const float y = F32 ? (float)v * scale : (float)((double)v * (double)scale);
        o[r] = (y + bi[r]) + po[r];
      }
      *reinterpret_cast<v4f*>(orow + n) = o;
    }
  }
}

__global__ void k_embed_qi8_cls(const float* __restrict__ cls, const float* __restrict__ pos, float* __restrict__ out,
                                int64_t images, int64_t hw, int64_t n) {
  const int64_t total = images * n, stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const int64_t img = i / n, c = i - img * n;
    out[img * (hw + 1) * n + c] = cls[c] + pos[c];
  }
}

}  // namespace
}  // namespace nqk

using namespace nqk;

extern "C" int nqk_im2col_q(const void* x, void* cols, int dtype, int64_t* rowsum, int64_t n, int64_t c, int64_t h,
                            int64_t w, int64_t kh, int64_t kw, int64_t ph0, int64_t pw0, int64_t sh, int64_t sw,
                            int64_t ho, int64_t wo, int64_t pad) {
  if (dtype < NQK_I8 || dtype > NQK_I64) return fail("nqk_im2col_q: integer storage (NQK_I8 .. NQK_I64) expected");
  if (n < 0 || c < 0 || h < 0 || w < 0 || ho < 0 || wo < 0) return fail("nqk_im2col_q: negative dimension");
  if (kh < 1 || kw < 1 || sh < 1 || sw < 1) return fail("nqk_im2col_q: kernel and strides of at least 1 expected");
  if (ph0 < 0 || pw0 < 0) return fail("nqk_im2col_q: negative padding");
  const int64_t lim = (int64_t)1 << 31;
  if (n >= lim || c >= lim || h >= lim || w >= lim || kh >= lim || kw >= lim || sh >= lim || sw >= lim || ph0 >= lim ||
      pw0 >= lim || ho >= lim || wo >= lim)
    return fail("nqk_im2col_q: dimension of 2^31 or more");
  const double in_total = (double)n * (double)c * (double)h * (double)w;
  const double out_total = (double)n * (double)ho * (double)wo * (double)kh * (double)kw * (double)c;
  if (in_total >= 4.0e18 || out_total >= 4.0e18) return fail("nqk_im2col_q: more than 2^62 elements");
  const int bits = dtype == NQK_I8 ? 8 : dtype == NQK_I16 ? 16 : dtype == NQK_I32 ? 32 : 64;
  if (bits < 64 && (pad < -((int64_t)1 << (bits - 1)) || pad > ((int64_t)1 << (bits - 1)) - 1))
    return fail("nqk_im2col_q: the pad value does not fit the storage dtype");
  const int64_t rows = n * ho * wo;
  if (rows <= 0 || kh * kw * c <= 0) return 0;
  if (!x || !cols) return fail("nqk_im2col_q: null pointer");
  const int esz = bits / 8;
  if ((((uintptr_t)x) | ((uintptr_t)cols)) & (uintptr_t)(esz - 1)) return fail("nqk_im2col_q: unaligned operands");
  if (rowsum && (((uintptr_t)rowsum) & 7)) return fail("nqk_im2col_q: unaligned row sums");
  const unsigned grid = grid_for(rows * 64);
  NQK_INT_DISPATCH(dtype, T,
                   hipLaunchKernelGGL(k_im2col_q<T>, dim3(grid), dim3(kThreads), 0, stream(), (const T*)x, (T*)cols,
                                      rowsum, n, c, h, w, kh, kw, ph0, pw0, sh, sw, ho, wo, pad));
  return launch_status("nqk_im2col_q");
}

extern "C" int nqk_embed_qi8(const int8_t* q, const int8_t* wt, const int32_t* colterm, float scale, int64_t zx,
                             int64_t w_l1max, const float* bias, const float* cls, const float* pos, float* out,
                             int64_t images, int64_t c, int64_t h, int64_t w, int64_t kh, int64_t kw, int64_t N) {
  if (images < 0 || N < 0 || c < 1 || h < 1 || w < 1) return fail("nqk_embed_qi8: non-positive dimension");
  if (kh != 16 || kw != 16) return fail("nqk_embed_qi8: 16 x 16 patches expected");
  if (h % 16 || w % 16) return fail("nqk_embed_qi8: the patches must tile the image (h % 16 == 0, w % 16 == 0)");
  if (N % 64) return fail("nqk_embed_qi8: N % 64 == 0 expected");
  if (c > (1 << 16) || h > (1 << 20) || w > (1 << 20) || images > (1 << 24) || N > (1 << 24))
    return fail("nqk_embed_qi8: dimension too large");
  const int64_t K = c * kh * kw;
  if (K % 64) return fail("nqk_embed_qi8: K % 64 == 0 expected");
  if (zx < -(1 << 20) || zx > (1 << 20)) return fail("nqk_embed_qi8: zero point out of range");
  const int64_t az = zx < 0 ? -zx : zx;
  // |acc| <= K 2^14 and |colterm| <= |zx| K 2^7: their difference must stay an int32
  if (K * ((int64_t)1 << 14) + az * K * ((int64_t)1 << 7) >= ((int64_t)1 << 31))
    return fail("nqk_embed_qi8: K 2^14 + |zx| K 2^7 reaches 2^31 (int32 accumulator)");
  if (images == 0 || N == 0) return 0;
  if (!q || !wt || !colterm || !bias || !cls || !pos || !out) return fail("nqk_embed_qi8: null pointer");
  if ((((uintptr_t)q) | ((uintptr_t)wt) | ((uintptr_t)colterm) | ((uintptr_t)bias) | ((uintptr_t)pos) |
       ((uintptr_t)out)) & 15)
    return fail("nqk_embed_qi8: unaligned operands (16 bytes)");
  if (((uintptr_t)cls) & 3) return fail("nqk_embed_qi8: unaligned class token");
  const int64_t wo = w / 16, hw = (h / 16) * wo, M = images * hw;
  if ((double)images * (double)c * (double)h * (double)w >= 4.0e18 || (double)(M + images) * (double)N >= 1.0e18)
    return fail("nqk_embed_qi8: tensor too large");
  const int wn = N % 128 == 0 ? 2 : 1;
  const int64_t tiles_n = N / (64 * wn), tiles = ((M + 127) / 128) * tiles_n;
  if (tiles > 2147483647) return fail("nqk_embed_qi8: grid too large");
  // f32 dequantize only where |acc - colterm| = |sum_k (x_k - zx) w_k| <= max|x - zx| * max_n sum_k |w_nk|
  // is proven below 2^24 (w_l1max < 0: unknown)
  const int64_t dx = (127 - zx > zx + 128) ? 127 - zx : zx + 128;
  const bool f32 = w_l1max >= 0 && w_l1max <= ((int64_t)1 << 24) && w_l1max * dx < ((int64_t)1 << 24);
  const int xcd = xcd_count();
  const dim3 grid((unsigned)tiles), block(256);
#define NQK_EQI8(WN_, F_)                                                                                          \
  hipLaunchKernelGGL((k_embed_qi8<WN_, F_>), grid, block, 0, stream(), q, wt, colterm, bias, pos, out, M, N, (int)c, \
                     hw, wo, h, w, scale, xcd, tiles_n)
  if (wn == 2) {
    if (f32) NQK_EQI8(2, true); else NQK_EQI8(2, false);
  } else {
    if (f32) NQK_EQI8(1, true); else NQK_EQI8(1, false);
  }
#undef NQK_EQI8
  if (int rc = launch_status("nqk_embed_qi8")) return rc;
  hipLaunchKernelGGL(k_embed_qi8_cls, dim3(grid_for(images * N)), dim3(kThreads), 0, stream(), cls, pos, out, images,
                     hw, N);
  return launch_status("nqk_embed_qi8(cls)");
}
