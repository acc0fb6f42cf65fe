// Key histogram and key range of a float32 array (streamed calibration, calibration.py).
//
//   key(x) = ~bits if the sign bit is set, else bits | 0x80000000     (nqk_glut.hip's okey)
//   bin(x) = key(x) >> NQK_HIST_SHIFT                                 (16384 bins: sign, exponent,
//                                                                      5 mantissa bits)
//   state  = int64 [NQK_HIST_BINS + 2]: counts, then the smallest and the largest key seen
// Everything is integer arithmetic on bit patterns and every update is an atomic add, min or
// max, so the state after a call does not depend on the order in which the lanes arrive.
//
// n > kHistDirectMax, with counts: every 256-lane workgroup keeps a uint32[16384] histogram in
// LDS (64 KiB and 64 bytes: two workgroups per CU), reads its share 16 bytes per lane through a
// grid-stride loop, kHistUnroll loads in flight per lane, counts with LDS atomic adds whose
// result is not used, and at the end adds its non-zero bins to the state with 64-bit global
// atomics.
// Below that size zeroing and flushing 16384 bins costs more than the data: the lanes add
// straight into the state.
// Both keys of zero (post-ReLU / post-GELU tensors are largely exact zeros, which would put every
// lane of a wave on one LDS word) are counted in a register per lane and added once per
// workgroup.  The key range is reduced across the workgroup first: at most one global atomicMin
// and atomicMax per workgroup (hist_block_end).
#include <stdlib.h>
#include "nqk_common.h"

namespace nqk {
namespace {

constexpr int kHistBins = NQK_HIST_BINS;
constexpr int kHistShift = NQK_HIST_SHIFT;
constexpr int64_t kHistDirectMax = NQK_HIST_DIRECT_MAX;
constexpr int kHistUnroll = 4;
// One launch takes at most this many elements (a multiple of 4, so the 16-byte phase of the
// pieces of one array stays the same).  An LDS counter and a lane's zero counters are 32 bits
// wide; a workgroup counts only elements of its own launch, which are fewer than 2^32 whatever
// the grid, so no counter can wrap.  The counts in the state are 64 bits.
constexpr int64_t kHistLaunchMax = (int64_t)1 << 31;
constexpr uint32_t kKeyNegZero = 0x7FFFFFFFu, kKeyPosZero = 0x80000000u;
static_assert(kHistBins == 1 << (32 - kHistShift), "bins cover the whole key");
static_assert((kKeyNegZero >> kHistShift) == kHistBins / 2 - 1 && (kKeyPosZero >> kHistShift) == kHistBins / 2, "zero bins");

__device__ __forceinline__ uint32_t hist_key(uint32_t u) { return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }

__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

struct HistLane {  // what one lane carries through its elements
  uint32_t mn = 0xFFFFFFFFu, mx = 0u, nzero = 0u, pzero = 0u;
};

// counts into `h` (LDS uint32 or global int64 words)
template <bool COUNTS, typename H>
__device__ __forceinline__ void hist_take(uint32_t bits, HistLane& l, H* h) {
  const uint32_t key = hist_key(bits);
  l.mn = key < l.mn ? key : l.mn;
  l.mx = key > l.mx ? key : l.mx;
  if (COUNTS) {
    if (key == kKeyNegZero) ++l.nzero;
    else if (key == kKeyPosZero) ++l.pzero;
    else atomicAdd(&h[key >> kHistShift], (H)1);
  }
}

// The workgroup's zero counts into `h` and its key range into the state, through `part` (16
// words of LDS): one atomic per workgroup and word at the most.  Thousands of waves on the two
// range words would take longer than the data (one address takes some 90 atomics per
// microsecond), so a workgroup first reads the word and leaves it alone unless it would move
// it: the words only ever move one way, so a stale read costs a needless atomic, never a missed
// one.  Every thread of the 256 calls it.
template <bool COUNTS, typename H>
__device__ __forceinline__ void hist_block_end(HistLane& l, H* h, int64_t* state, uint32_t* part) {
  for (int off = 32; off > 0; off >>= 1) {
    const uint32_t a = __shfl_xor(l.mn, off, 64), b = __shfl_xor(l.mx, off, 64);
    l.mn = a < l.mn ? a : l.mn;
    l.mx = b > l.mx ? b : l.mx;
  }
  const uint32_t nz = COUNTS ? wave_sum_u32(l.nzero) : 0, pz = COUNTS ? wave_sum_u32(l.pzero) : 0;
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    part[w] = l.mn;
    part[4 + w] = l.mx;
    part[8 + w] = nz;
    part[12 + w] = pz;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t mn = part[0], mx = part[4], bnz = part[8], bpz = part[12];
    for (int i = 1; i < 4; ++i) {
      mn = part[i] < mn ? part[i] : mn;
      mx = part[4 + i] > mx ? part[4 + i] : mx;
      bnz += part[8 + i];
      bpz += part[12 + i];
    }
    if (COUNTS) {
      if (bnz) atomicAdd(&h[kKeyNegZero >> kHistShift], (H)bnz);
      if (bpz) atomicAdd(&h[kKeyPosZero >> kHistShift], (H)bpz);
    }
    if (mn <= mx) {  // the workgroup saw an element; keys are below 2^32, so signed == unsigned order
      unsigned long long* lo = reinterpret_cast<unsigned long long*>(state + kHistBins);
      if (mn < __hip_atomic_load(lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(lo, (unsigned long long)mn);
      if (mx > __hip_atomic_load(lo + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(lo + 1, (unsigned long long)mx);
    }
  }
  __syncthreads();
}

// x[0..head) and x[head + 4 * nvec .. n) element-wise (head, tail <= 3: block 0's first lanes),
// the nvec 16-byte groups between them grid-stride.
template <bool COUNTS>
__global__ void __launch_bounds__(256)
k_hist_lds(const uint32_t* __restrict__ x, int64_t n, int head, int64_t nvec, int64_t* __restrict__ state) {
  __shared__ __attribute__((aligned(16))) uint32_t h[COUNTS ? kHistBins : 4];
  __shared__ uint32_t part[16];
  if (COUNTS) {
    for (int i = threadIdx.x; i < kHistBins / 4; i += 256) reinterpret_cast<uint4*>(h)[i] = make_uint4(0, 0, 0, 0);
    __syncthreads();
  }
  HistLane l;
  const uint4* xv = reinterpret_cast<const uint4*>(x + head);
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t g0 = (int64_t)blockIdx.x * 256 + threadIdx.x; g0 < nvec; g0 += stride * kHistUnroll) {
    uint4 v[kHistUnroll] = {};
#pragma unroll
    for (int u = 0; u < kHistUnroll; ++u) {
      const int64_t g = g0 + u * stride;
      if (g < nvec) v[u] = xv[g];
    }
#pragma unroll
    for (int u = 0; u < kHistUnroll; ++u) {
      if (g0 + u * stride < nvec) {
        hist_take<COUNTS>(v[u].x, l, h);
        hist_take<COUNTS>(v[u].y, l, h);
        hist_take<COUNTS>(v[u].z, l, h);
        hist_take<COUNTS>(v[u].w, l, h);
      }
    }
  }
  if (blockIdx.x == 0) {
    const int64_t tail0 = head + 4 * nvec;
    if ((int)threadIdx.x < head) hist_take<COUNTS>(x[threadIdx.x], l, h);
    if (tail0 + threadIdx.x < n) hist_take<COUNTS>(x[tail0 + threadIdx.x], l, h);  // n - tail0 <= 3
  }
  hist_block_end<COUNTS>(l, h, state, part);
  if (COUNTS) {
    for (int b = threadIdx.x; b < kHistBins; b += 256) {
      const uint32_t c = h[b];
      if (c) atomicAdd(reinterpret_cast<unsigned long long*>(state + b), (unsigned long long)c);
    }
  }
}

template <bool COUNTS>
__global__ void __launch_bounds__(256)
k_hist_direct(const uint32_t* __restrict__ x, int64_t n, int64_t* __restrict__ state) {
  __shared__ uint32_t part[16];
  HistLane l;
  unsigned long long* h = reinterpret_cast<unsigned long long*>(state);
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) hist_take<COUNTS>(x[i], l, h);
  hist_block_end<COUNTS>(l, h, state, part);
}

int hist_cus() {
  static int n = 0;
  if (n == 0) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0)
      n = 256;
  }
  return n;
}

// NQK_HIST_DIRECT_MAX=<elements> moves the switch-over (read on every call: the benchmark
// times both kernels at one size with it; the result does not depend on it)
int64_t hist_direct_max() {
  const char* e = getenv("NQK_HIST_DIRECT_MAX");
  return e && *e ? atoll(e) : kHistDirectMax;
}

void launch_hist(const float* x, int64_t n, int64_t* state, bool counts) {
  const uint32_t* xb = reinterpret_cast<const uint32_t*>(x);
  if (n <= hist_direct_max()) {
    const dim3 grid(grid_for(n)), block(256);
    if (counts) hipLaunchKernelGGL(k_hist_direct<true>, grid, block, 0, stream(), xb, n, state);
    else hipLaunchKernelGGL(k_hist_direct<false>, grid, block, 0, stream(), xb, n, state);
    return;
  }
  int64_t head = (int64_t)((16 - ((uintptr_t)x & 15)) & 15) / 4;  // x is 4-byte aligned
  if (head > n) head = n;
  const int64_t nvec = (n - head) / 4;
  // two workgroups per CU hold their 64 KiB histograms side by side; without counts there is no
  // LDS and eight per CU keep more loads in flight
  const int64_t cap = (int64_t)(counts ? 2 : 8) * hist_cus();
  const dim3 grid(grid_for(nvec, 256, cap)), block(256);
  if (counts) hipLaunchKernelGGL(k_hist_lds<true>, grid, block, 0, stream(), xb, n, (int)head, nvec, state);
  else hipLaunchKernelGGL(k_hist_lds<false>, grid, block, 0, stream(), xb, n, (int)head, nvec, state);
}

}  // namespace
}  // namespace nqk

using namespace nqk;

extern "C" int nqk_hist_f32(const float* x, int64_t n, int64_t* state, int counts) {
  if (n < 0) return fail("nqk_hist_f32: n < 0");
  if (n > NQK_HIST_MAX_N) return fail("nqk_hist_f32: n above NQK_HIST_MAX_N (2^40)");
  if (!x || !state) return fail("nqk_hist_f32: null pointer");
  if ((uintptr_t)x % 4 || (uintptr_t)state % 8) return fail("nqk_hist_f32: x needs 4-byte, state 8-byte alignment");
  for (int64_t at = 0; at < n; at += kHistLaunchMax)
    launch_hist(x + at, n - at < kHistLaunchMax ? n - at : kHistLaunchMax, state, counts != 0);
  return n ? launch_status("nqk_hist_f32") : 0;
}
