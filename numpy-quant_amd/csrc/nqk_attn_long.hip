// Fused self-attention for sequences longer than nqk_attention_fused takes (225 tokens and up:
// ViT/16 at 240 px = 226, 384 px = 577, 512 px = 1025), nqk_attention_long.
//
// nqk_attention_fused keeps a query row's whole score row in registers; here the score rows of a
// block of 16 queries live in LDS.  One workgroup (four waves) per (image, head, 16 query rows):
//   1. S^T = K Q^T     v_mfma_i32_16x16x64_i8, K rows straight from L2 as the A operand (every
//                      query block of a head reads the same K: the blocks of a head are neighbours
//                      on one XCD, xcd_remap), a second MFMA against an all-ones operand gives the K
//                      row sums of the zero-point term in the accumulator layout; dequantize + Div
//                      (EPI_SCORES) -> f32 score block [16][TP + 4] in LDS
//   2. softmax         one wave per row, as k_softmax_quant: max, NumPy exp, NumPy pairwise sum by
//                      the general plan (PwPlan / wave_pairwise_sum: any depth of the recursion),
//                      divide, quantize -> int8 P block [16][TP + 16] in LDS, pad columns 0, row sums
//   3. V^T             staged over the dead score block (4 x 4 byte transposes, as k_attention)
//   4. ctx^T = V^T P^T v_mfma_i32_16x16x64_i8, wave w takes head dimensions 16 w .. 16 w + 15;
//                      dequantize, quantize (EPI_PV), 4 dimensions of a query row per store
// Every element goes through exactly the operations of nqk_qgemm_fused EPI_SCORES ->
// nqk_softmax_quant -> nqk_qgemm_fused EPI_PV (the int32 zero-point algebra is exact: host check;
// div_rc / quant_zp are nqk_fused.hip's, subnormal fallback included), so ctx is bit-identical to
// that chain.  The only substitution is np_expf_nonpos for np_expf on the arguments y - max <= 0,
// equal on every such input (nqk_selftest_fastmath, counts[2]); a normal s_qk (host check) keeps
// every score finite.
//
// LDS for TP = tokens rounded up to 64: 64 (TP + 16) score block / V^T + 16 (TP + 16) P +
// the four waves' pairwise-sum scratch + column terms = 80 TP + 10 880 bytes: 60.6 KiB at 577 tokens
// (two workgroups per CU), 95.6 KiB at 1025, and TP = 1856 is the most that fits 160 KiB
// (NQK_ATTN_LONG_MAX_T).
#include "nqk_common.h"
#include "nqk_numerics.h"

namespace nqk {
namespace {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef float v4f __attribute__((ext_vector_type(4)));

constexpr int AL_QB = 16;                                  // query rows per workgroup
constexpr int AL_WS = kMaxLeaves * 8 + kMaxLeaves + 4;     // floats of wave_pairwise_sum scratch per wave
constexpr int AL_LDS_MAX = 160 * 1024;
__host__ __device__ constexpr int al_tp(int T) { return (T + 63) / 64 * 64; }
__host__ __device__ constexpr size_t al_lds(int T) {
  return (size_t)64 * (al_tp(T) + 16) + (size_t)AL_QB * (al_tp(T) + 16) + (size_t)4 * AL_WS * 4 + 64 * 4 + AL_QB * 4;
}
static_assert(al_lds(NQK_ATTN_LONG_MAX_T) <= AL_LDS_MAX && al_lds(NQK_ATTN_LONG_MAX_T + 1) > AL_LDS_MAX,
              "NQK_ATTN_LONG_MAX_T is the largest token count whose workgroup fits the CU's LDS");

struct LongArgs {
  int T, TP, QR, NQB, H, ld_out, xcds;
  int zq, zk, zp, zv;  // zero points (host-checked: every int32 intermediate is exact)
  int kq, kp;          // zq*zk*64, zp*zv*T
  float s_qk, div, s_p, s_pv, s_ctx;
  double rdiv, rs_p, zp_p, rs_ctx, zp_ctx, lo, hi;
};

__device__ __forceinline__ int sum16l(v4i c) {
  int s = __builtin_amdgcn_sdot4(c[0], 0x01010101, 0, false);
  s = __builtin_amdgcn_sdot4(c[1], 0x01010101, s, false);
  s = __builtin_amdgcn_sdot4(c[2], 0x01010101, s, false);
  return __builtin_amdgcn_sdot4(c[3], 0x01010101, s, false);
}

// nqk_fused.hip's div_rc / quant_zp (the chain's own arithmetic)
__device__ __forceinline__ float div_rc_l(float x, float c, double rc) {
  const float t = (float)((double)x * rc);
  return __builtin_fabsf(t) < 0x1p-125f ? x / c : t;
}
__device__ __forceinline__ int quant_zp_l(float x, float s, double rs, double zp, double lo, double hi) {
  const float t = div_rc_l(x, s, rs);
  double u = zp + (double)t;
  if (u != u) return (int)lo;
  u = u < lo ? lo : u;
  u = u > hi ? hi : u;
  return (int)__builtin_rint(u);
}

__global__ void __launch_bounds__(256)
k_attn_long(const int8_t* __restrict__ Qg, const int8_t* __restrict__ Kg, const int8_t* __restrict__ Vg,
            int8_t* __restrict__ ctx, LongArgs a, PwPlan p) {
  extern __shared__ __attribute__((aligned(16))) int8_t lds[];
  const int T = a.T, TP = a.TP, SST = TP + 4, PST = TP + 16;
  float* const S = reinterpret_cast<float*>(lds);  // [16][SST] f32 scores, then exp values
  int8_t* const Vt = lds;                          // [64][PST] int8 V^T over the dead score block
  int8_t* const P = lds + 64 * PST;                // [16][PST] int8 probabilities
  float* const scr = reinterpret_cast<float*>(P + AL_QB * PST);
  int* const colV = reinterpret_cast<int*>(scr + 4 * AL_WS);  // colsum(V[:, d]) * zp - zp*zv*T
  int* const rps = colV + 64;                                 // row sums of P
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l15 = lane & 15, g = lane >> 4;
  // tile = (image, head) major, query block minor: a head's blocks share an XCD's L2 for K and V
  const int tile = xcd_remap<int>((int)blockIdx.x, (int)gridDim.x, a.xcds);
  const int bh = tile / a.NQB, m0 = (tile - bh * a.NQB) * AL_QB;
  const int img = bh / a.H, head = bh - img * a.H;
  const int8_t* q = Qg + (int64_t)bh * T * 64;
  const int8_t* k = Kg + (int64_t)bh * T * 64;
  const int8_t* v = Vg + (int64_t)bh * T * 64;

  // ---- 1. scores: tile c = keys 16 c .. 16 c + 15 against the block's 16 queries; the accumulator
  // of lane (l15, g) holds keys 16 c + 4 g + r (r < 4) of query m0 + l15
  {
    const int mq = min(m0 + l15, T - 1);  // (rows past the last token: a copy of it, never stored)
    const v4i qf = *reinterpret_cast<const v4i*>(q + mq * 64 + g * 16);
    int rq = sum16l(qf);
    rq += __shfl_xor(rq, 16, 64);
    rq += __shfl_xor(rq, 32, 64);
    const int rowterm = rq * a.zk;
    const v4i ones = {0x01010101, 0x01010101, 0x01010101, 0x01010101};
    const int NT = (T + 15) >> 4;
    v4i kn = *reinterpret_cast<const v4i*>(k + min(16 * wave + l15, T - 1) * 64 + g * 16);
    for (int c = wave; c < NT; c += 4) {
      const v4i kf = kn;
      kn = *reinterpret_cast<const v4i*>(k + min(16 * (c + 4) + l15, T - 1) * 64 + g * 16);
      const v4i z = {0, 0, 0, 0};
      const v4i acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(kf, qf, z, 0, 0, 0);
      const v4i ks = __builtin_amdgcn_mfma_i32_16x16x64_i8(kf, ones, z, 0, 0, 0);  // rowsum(K[key])
      v4f y;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int vv = acc[r] - rowterm - (ks[r] * a.zq - a.kq);
        const float d = (float)((double)vv * (double)a.s_qk);
        y[r] = div_rc_l(d, a.div, a.rdiv);
      }
      *reinterpret_cast<v4f*>(S + l15 * SST + 16 * c + 4 * g) = y;
    }
  }
  __syncthreads();

  // ---- 2. softmax + quantize, one wave per row (k_softmax_quant); a lane takes 4 columns at once
  {
    float* const part = scr + wave * AL_WS;
    float* const leafv = part + kMaxLeaves * 8;
    const int n4 = TP >> 2;
    for (int r = wave; r < AL_QB && m0 + r < a.QR; r += 4) {
      float* const vr = S + r * SST;
      float mx = -__builtin_inff();
      for (int i = lane; i < n4; i += 64) {
        const v4f t = *reinterpret_cast<const v4f*>(vr + 4 * i);
#pragma unroll
        for (int j = 0; j < 4; ++j) mx = (4 * i + j < T && t[j] > mx) ? t[j] : mx;
      }
      for (int off = 32; off > 0; off >>= 1) {
        const float o = __shfl_xor(mx, off, 64);
        mx = o > mx ? o : mx;
      }
      const float nm = -mx;
      for (int i = lane; i < n4; i += 64) {
        v4f t = *reinterpret_cast<const v4f*>(vr + 4 * i);
#pragma unroll
        for (int j = 0; j < 4; ++j) t[j] = 4 * i + j < T ? np_expf_nonpos(t[j] + nm) : 0.0f;
        *reinterpret_cast<v4f*>(vr + 4 * i) = t;
      }
      wave_lds_sync();
      const float ssum = wave_pairwise_sum(vr, p, part, leafv);
      const double rsum = 1.0 / (double)ssum;
      int rp = 0;
      for (int i = lane; i < n4; i += 64) {
        const v4f t = *reinterpret_cast<const v4f*>(vr + 4 * i);
        uint32_t packed = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          int qv = quant_zp_l(div_rc_l(t[j], ssum, rsum), a.s_p, a.rs_p, a.zp_p, a.lo, a.hi);
          qv = 4 * i + j < T ? qv : 0;  // pad columns: 0
          rp += qv;
          packed |= (uint32_t)(qv & 0xff) << (8 * j);
        }
        *reinterpret_cast<uint32_t*>(P + r * PST + 4 * i) = packed;
      }
      for (int off = 32; off > 0; off >>= 1) rp += __shfl_xor(rp, off, 64);
      if (lane == 0) rps[r] = rp;
    }
  }
  __syncthreads();

  // ---- 3. V^T (zero padded to TP tokens) over the score block: blocks of 4 tokens x 16 dims, a
  // 4 x 4 byte transpose per dword column, sixteen 4-byte writes
  for (int blk = tid; blk < TP; blk += 256) {  // TP / 4 token blocks x 4 dim chunks
    const int c = blk / (TP / 4), rb = blk - c * (TP / 4);
    v4i w[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int tok = 4 * rb + r;
      w[r] = tok < T ? *reinterpret_cast<const v4i*>(v + tok * 64 + c * 16) : v4i{0, 0, 0, 0};
    }
#pragma unroll
    for (int gq = 0; gq < 4; ++gq) {
      const uint32_t lo01 = __builtin_amdgcn_perm((uint32_t)w[1][gq], (uint32_t)w[0][gq], 0x05010400u);
      const uint32_t hi01 = __builtin_amdgcn_perm((uint32_t)w[1][gq], (uint32_t)w[0][gq], 0x07030602u);
      const uint32_t lo23 = __builtin_amdgcn_perm((uint32_t)w[3][gq], (uint32_t)w[2][gq], 0x05010400u);
      const uint32_t hi23 = __builtin_amdgcn_perm((uint32_t)w[3][gq], (uint32_t)w[2][gq], 0x07030602u);
      const uint32_t o[4] = {__builtin_amdgcn_perm(lo23, lo01, 0x05040100u), __builtin_amdgcn_perm(lo23, lo01, 0x07060302u),
                             __builtin_amdgcn_perm(hi23, hi01, 0x05040100u), __builtin_amdgcn_perm(hi23, hi01, 0x07060302u)};
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) *reinterpret_cast<uint32_t*>(Vt + (16 * c + 4 * gq + kk) * PST + 4 * rb) = o[kk];
    }
  }
  __syncthreads();
  {
    const int d = tid >> 2, part = tid & 3;
    int s = 0;
    for (int c = part; c < TP / 16; c += 4) s += sum16l(*reinterpret_cast<const v4i*>(Vt + d * PST + c * 16));
    s += __shfl_xor(s, 1, 64);
    s += __shfl_xor(s, 2, 64);
    if (part == 0) colV[d] = s * a.zp - a.kp;
  }
  __syncthreads();

  // ---- 4. ctx^T = V^T P^T: the accumulator of lane (l15, g) holds head dimensions 16 wave + 4 g + r
  // of query m0 + l15 (two accumulators: two independent MFMA chains)
  {
    const v4i z = {0, 0, 0, 0};
    v4i acc0 = z, acc1 = z;
    const int8_t* const va = Vt + (16 * wave + l15) * PST + 16 * g;
    const int8_t* const pb = P + l15 * PST + 16 * g;
    const int NC = TP >> 6;
    for (int ch = 0; ch < NC; ch += 2) {
      acc0 = __builtin_amdgcn_mfma_i32_16x16x64_i8(*reinterpret_cast<const v4i*>(va + 64 * ch),
                                                   *reinterpret_cast<const v4i*>(pb + 64 * ch), acc0, 0, 0, 0);
      if (ch + 1 < NC)
        acc1 = __builtin_amdgcn_mfma_i32_16x16x64_i8(*reinterpret_cast<const v4i*>(va + 64 * ch + 64),
                                                     *reinterpret_cast<const v4i*>(pb + 64 * ch + 64), acc1, 0, 0, 0);
    }
    const int m = m0 + l15;
    const int rowp = rps[l15] * a.zv;
    const int d0 = 16 * wave + 4 * g;
    const v4i cv = *reinterpret_cast<const v4i*>(colV + d0);
    uint32_t packed = 0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int vv = (acc0[r] + acc1[r]) - rowp - cv[r];
      const float o = (float)((double)vv * (double)a.s_pv);
      const int qv = quant_zp_l(o, a.s_ctx, a.rs_ctx, a.zp_ctx, a.lo, a.hi);
      packed |= (uint32_t)(qv & 0xff) << (8 * r);
    }
    if (m < a.QR) *reinterpret_cast<uint32_t*>(ctx + ((int64_t)img * T + m) * a.ld_out + head * 64 + d0) = packed;
  }
}

}  // namespace
}  // namespace nqk

using namespace nqk;

extern "C" int nqk_attention_long(const int8_t* q, const int8_t* k, const int8_t* v, int8_t* ctx,
                                  int64_t batch_heads, const nqk_attention* p) {
  // every refusal comes before any launch
  if (p == nullptr) return fail("nqk_attention_long: null parameters");
  if (batch_heads < 0) return fail("nqk_attention_long: negative batch_heads");
  const int T = p->tokens;
  if (p->hdim != 64) return fail("nqk_attention_long: head dimension 64 expected");
  if (T < NQK_ATTN_LONG_MIN_T || T > NQK_ATTN_LONG_MAX_T)
    return fail("nqk_attention_long: 225 <= tokens <= NQK_ATTN_LONG_MAX_T expected (nqk_attention_fused below)");
  if (p->q_rows < 0 || p->q_rows > T) return fail("nqk_attention_long: 0 <= q_rows <= tokens expected");
  if (p->heads < 1 || batch_heads % p->heads) return fail("nqk_attention_long: batch_heads % heads != 0");
  if (p->ld_out < p->heads * 64) return fail("nqk_attention_long: ld_out < heads * 64");
  if (p->bit_width < 2 || p->bit_width > 8) return fail("nqk_attention_long: 2 <= bit_width <= 8 expected");
  if (q == nullptr || k == nullptr || v == nullptr || ctx == nullptr) return fail("nqk_attention_long: null Q / K / V / ctx");
  if ((((uintptr_t)q) | ((uintptr_t)k) | ((uintptr_t)v)) & 15) return fail("nqk_attention_long: unaligned Q/K/V");
  if ((((uintptr_t)ctx) & 3) || (p->ld_out & 3)) return fail("nqk_attention_long: ctx / ld_out not 4-byte aligned");
  auto small = [](int64_t z, int64_t lim) { return z >= -lim && z <= lim; };
  if (!small(p->zq, 4096) || !small(p->zk, 4096) || !small(p->zp_p, 1024) || !small(p->zv, 1024))
    return fail("nqk_attention_long: zero points beyond the int32-exact range");
  // int32 algebra: |acc| + |row term| + |column term| + |constant| for int8 operands (|x| <= 128),
  // over 64 head dimensions for the scores and over T tokens for the context
  const double bs = 64.0 * (16384.0 + 128.0 * (double)(llabs(p->zq) + llabs(p->zk)) + (double)llabs(p->zq * p->zk));
  const double bp = (double)T * (16384.0 + 128.0 * (double)(llabs(p->zp_p) + llabs(p->zv)) + (double)llabs(p->zp_p * p->zv));
  if (!(bs < 2147483648.0) || !(bp < 2147483648.0))
    return fail("nqk_attention_long: zero points beyond the int32-exact range at this token count");
  auto normal = [](float x) { return __builtin_fabsf(x) >= 0x1p-100f && __builtin_fabsf(x) <= 0x1p100f; };
  if (!normal(p->s_p) || !normal(p->s_ctx) || !normal(p->div) || !normal(p->s_qk) || !normal(p->s_pv))
    return fail("nqk_attention_long: scales / divisor outside [2^-100, 2^100]");
  const int QR = p->q_rows ? p->q_rows : T;
  const int nqb = (QR + AL_QB - 1) / AL_QB;
  if (batch_heads * nqb > 0x7fffffff) return fail("nqk_attention_long: too many workgroups");
  if (batch_heads == 0) return 0;
  PwPlan plan;
  if (row_plan(T, plan)) return -1;
  LongArgs a{};
  a.T = T;
  a.TP = al_tp(T);
  a.QR = QR;
  a.NQB = nqb;
  a.H = p->heads;
  a.ld_out = p->ld_out;
  a.xcds = xcd_count();
  a.zq = (int)p->zq;
  a.zk = (int)p->zk;
  a.zp = (int)p->zp_p;
  a.zv = (int)p->zv;
  a.kq = a.zq * a.zk * 64;
  a.kp = a.zp * a.zv * T;
  a.s_qk = p->s_qk;
  a.div = p->div;
  a.rdiv = 1.0 / (double)p->div;
  a.s_p = p->s_p;
  a.rs_p = 1.0 / (double)p->s_p;
  a.zp_p = (double)p->zp_p;
  a.s_pv = p->s_pv;
  a.s_ctx = p->s_ctx;
  a.rs_ctx = 1.0 / (double)p->s_ctx;
  a.zp_ctx = (double)p->zp_ctx;
  a.lo = -__builtin_ldexp(1.0, p->bit_width - 1);
  a.hi = __builtin_ldexp(1.0, p->bit_width - 1) - 1.0;
  const size_t shm = al_lds(T);
  static bool lds_attr = false;  // the workgroup may ask for more than the 64 KiB default of dynamic LDS
  if (!lds_attr) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(k_attn_long), hipFuncAttributeMaxDynamicSharedMemorySize,
                            AL_LDS_MAX) != hipSuccess)
      (void)hipGetLastError();
    lds_attr = true;
  }
  const dim3 grid((unsigned)(batch_heads * nqb));
  hipLaunchKernelGGL(k_attn_long, grid, dim3(256), shm, stream(), q, k, v, ctx, a, plan);
  return launch_status("nqk_attention_long");
}
