// Per-channel absolute maxima of a float32 matrix (channel equalization, equalize.py).
//
//   key(v)  = bits(v) & 0x7FFFFFFF, every NaN -> 0x7FC00000      (uint32, monotone in |v|, NaN on top)
//   axis 0:   state[c] = umax(state[c], key(x[r][c])) over all r
//   axis 1:   state[r] = umax(state[r], key(x[r][c])) over all c
// The state read back as float32 is np.abs(x).max(axis), NaN included.  Everything is an integer
// maximum of bit patterns, in registers, in LDS and as a global atomicMax, so the state after a call
// depends neither on the grid nor on the order in which the lanes arrive.  A fresh state is zero.
//
// axis 0: a workgroup of 256 owns a strip of columns and a chunk of rows.  CW lanes lie across the
// strip, each on VEC consecutive columns (VEC = 4: one 16-byte load), the other 256 / CW lanes of a
// column take every (256 / CW)-th row of the chunk, kUnroll loads in flight.  The lanes' maxima are
// folded through LDS and every column of the strip gets at most one global atomic per workgroup: a
// workgroup first reads the word and leaves it alone unless it would move it (the words only grow,
// so a stale read costs a needless atomic, never a missed one).
// 16-byte loads need every row on the same 16-byte phase (ld % 4 == 0); the columns before the first
// aligned one and after the last whole group go through the 4-column scalar instance.
// axis 1: a wave per row, or per segment of a row when there are few rows (grid-stride), 16-byte
// loads between a scalar head and tail, a DPP fold inside each row of 16 lanes and two exchanges
// across them, one atomic per wave.
#include "nqk_common.h"

namespace nqk {
namespace {

constexpr int kUnroll = 4;
constexpr uint32_t kNanKey = 0x7FC00000u;

__device__ __forceinline__ uint32_t abs_key(uint32_t u) {
  const uint32_t k = u & 0x7FFFFFFFu;
  return k > 0x7F800000u ? kNanKey : k;
}
__device__ __forceinline__ uint32_t umax(uint32_t a, uint32_t b) { return a > b ? a : b; }

__device__ __forceinline__ void state_max(uint32_t* p, uint32_t m) {
  if (m > __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(p, m);
}

template <int VEC> struct Ld;
template <> struct Ld<1> { using T = uint32_t; };
template <> struct Ld<4> { using T = uint4; };
__device__ __forceinline__ void take(uint32_t (&m)[1], uint32_t v) { m[0] = umax(m[0], abs_key(v)); }
__device__ __forceinline__ void take(uint32_t (&m)[4], const uint4& v) {
  m[0] = umax(m[0], abs_key(v.x));
  m[1] = umax(m[1], abs_key(v.y));
  m[2] = umax(m[2], abs_key(v.z));
  m[3] = umax(m[3], abs_key(v.w));
}

// x: the first column of the range, ncols of them (a multiple of VEC), rows of ld elements;
// blockIdx.x: the strip of CW * VEC columns, blockIdx.y: the chunk of chunk_rows rows.
template <int VEC, int CW>
__global__ void __launch_bounds__(256)
k_absmax_cols(const uint32_t* __restrict__ x, int64_t rows, int64_t ncols, int64_t ld, int64_t chunk_rows,
              uint32_t* __restrict__ state) {
  constexpr int R = 256 / CW, SW = CW * VEC;
  using T = typename Ld<VEC>::T;
  __shared__ uint32_t part[R * SW];
  const int tc = threadIdx.x % CW, tr = threadIdx.x / CW;
  const int64_t c0 = (int64_t)blockIdx.x * SW;
  const int64_t c = c0 + (int64_t)tc * VEC;
  const int64_t r0 = (int64_t)blockIdx.y * chunk_rows;
  const int64_t r1 = r0 + chunk_rows < rows ? r0 + chunk_rows : rows;
  uint32_t m[VEC] = {};
  if (c < ncols) {  // ncols is a multiple of VEC: c + VEC <= ncols
    const uint32_t* col = x + c;
    for (int64_t r = r0 + tr; r < r1; r += (int64_t)R * kUnroll) {
      T v[kUnroll] = {};
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const int64_t ru = r + (int64_t)u * R;
        if (ru < r1) v[u] = *reinterpret_cast<const T*>(col + ru * ld);
      }
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) take(m, v[u]);  // a row not loaded is +0: key 0
    }
  }
#pragma unroll
  for (int j = 0; j < VEC; ++j) part[tr * SW + tc * VEC + j] = m[j];
  __syncthreads();
  for (int s = threadIdx.x; s < SW; s += 256) {
    uint32_t mx = part[s];
#pragma unroll 4
    for (int j = 1; j < R; ++j) mx = umax(mx, part[j * SW + s]);
    if (c0 + s < ncols) state_max(state + c0 + s, mx);
  }
}

template <int CTRL>
__device__ __forceinline__ uint32_t dpp_max(uint32_t v) {
  return umax(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xF, 0xF, false));
}

// wave `wi` of the grid takes segment wi % nseg of row wi / nseg: segw columns from seg * segw on
__global__ void __launch_bounds__(256)
k_absmax_rows(const uint32_t* __restrict__ x, int64_t rows, int64_t cols, int64_t ld, int64_t segw, int64_t nseg,
              uint32_t* __restrict__ state) {
  const int lane = threadIdx.x & 63;
  const int64_t waves = (int64_t)gridDim.x * 4, work = rows * nseg;
  for (int64_t wi = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); wi < work; wi += waves) {
    const int64_t r = wi / nseg, c0 = (wi % nseg) * segw;
    const int64_t n = cols - c0 < segw ? cols - c0 : segw;
    const uint32_t* row = x + r * ld + c0;
    int64_t head = (int64_t)((16 - ((uintptr_t)row & 15)) & 15) / 4;  // row is 4-byte aligned
    if (head > n) head = n;
    const int64_t nvec = (n - head) / 4, tail0 = head + 4 * nvec;
    uint32_t m[4] = {};
    if (lane < head) m[0] = abs_key(row[lane]);
    if (tail0 + lane < n) m[1] = abs_key(row[tail0 + lane]);  // n - tail0 <= 3
    const uint4* rv = reinterpret_cast<const uint4*>(row + head);
    for (int64_t g = lane; g < nvec; g += 64 * kUnroll) {
      uint4 v[kUnroll] = {};
#pragma unroll
      for (int u = 0; u < kUnroll; ++u)
        if (g + u * 64 < nvec) v[u] = rv[g + u * 64];
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) take(m, v[u]);
    }
    uint32_t mx = umax(umax(m[0], m[1]), umax(m[2], m[3]));
    mx = dpp_max<0xB1>(mx);   // quad_perm [1,0,3,2]
    mx = dpp_max<0x4E>(mx);   // quad_perm [2,3,0,1]
    mx = dpp_max<0x141>(mx);  // row_half_mirror
    mx = dpp_max<0x140>(mx);  // row_mirror: the 16 lanes of a row agree
    mx = umax(mx, (uint32_t)__shfl_xor((int)mx, 16, 64));
    mx = umax(mx, (uint32_t)__shfl_xor((int)mx, 32, 64));
    if (lane == 0) state_max(state + r, mx);
  }
}

int absmax_cus() {
  static int n = 0;
  if (n == 0) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0)
      n = 256;
  }
  return n;
}

// columns [c_first, c_first + ncols) of x through instance <VEC, CW>
template <int VEC, int CW>
void launch_cols(const uint32_t* x, int64_t rows, int64_t c_first, int64_t ncols, int64_t ld, uint32_t* state) {
  if (ncols <= 0) return;
  constexpr int R = 256 / CW, SW = CW * VEC;
  const int64_t strips = (ncols + SW - 1) / SW;
  // four workgroups per CU over the whole grid; a chunk is at least one pass of the unrolled loop
  int64_t chunks = ((int64_t)4 * absmax_cus() + strips - 1) / strips;
  const int64_t most = (rows + (int64_t)R * kUnroll - 1) / ((int64_t)R * kUnroll);
  if (chunks > most) chunks = most;
  if (chunks > 65535) chunks = 65535;
  if (chunks < 1) chunks = 1;
  const int64_t chunk_rows = (rows + chunks - 1) / chunks;
  chunks = (rows + chunk_rows - 1) / chunk_rows;
  // strips of one launch stay below 2^31 / SW columns
  const dim3 grid((unsigned)strips, (unsigned)chunks), block(256);
  hipLaunchKernelGGL((k_absmax_cols<VEC, CW>), grid, block, 0, stream(), x + c_first, rows, ncols, ld, chunk_rows,
                     state + c_first);
}

}  // namespace
}  // namespace nqk

using namespace nqk;

extern "C" int nqk_absmax_f32(const float* x, int64_t rows, int64_t cols, int64_t ld, int axis, uint32_t* state) {
  if (rows < 0 || cols < 0 || ld < 0) return fail("nqk_absmax_f32: negative size");
  if (cols > ld) return fail("nqk_absmax_f32: cols > ld");
  if (axis != 0 && axis != 1) return fail("nqk_absmax_f32: axis must be 0 or 1");
  if (!x || !state) return fail("nqk_absmax_f32: null pointer");
  if ((uintptr_t)x % 4 || (uintptr_t)state % 4) return fail("nqk_absmax_f32: x and state need 4-byte alignment");
  if (cols > ((int64_t)1 << 31) || rows > ((int64_t)1 << 40))
    return fail("nqk_absmax_f32: more than 2^31 columns or 2^40 rows");
  if (rows == 0 || cols == 0) return 0;
  const uint32_t* xb = reinterpret_cast<const uint32_t*>(x);
  if (axis == 1) {
    // a wave per row; few rows are cut into segments of at least 256 columns (a multiple of 4, so
    // every segment keeps its row's 16-byte phase) until some four waves per SIMD exist
    const int64_t want = ((int64_t)16 * absmax_cus() + rows - 1) / rows, most = (cols + 255) / 256;
    int64_t nseg = want < most ? want : most;
    const int64_t segw = ((cols + nseg - 1) / nseg + 3) / 4 * 4;
    nseg = (cols + segw - 1) / segw;
    const int64_t blocks = (rows * nseg + 3) / 4, cap = (int64_t)8 * absmax_cus();
    hipLaunchKernelGGL(k_absmax_rows, dim3((unsigned)(blocks < cap ? blocks : cap)), dim3(256), 0, stream(), xb, rows,
                       cols, ld, segw, nseg, state);
    return launch_status("nqk_absmax_f32");
  }
  int64_t head = (int64_t)((16 - ((uintptr_t)x & 15)) & 15) / 4;
  if (ld % 4 == 0 && cols - head >= 4) {
    const int64_t body = (cols - head) / 4 * 4;
    launch_cols<1, 4>(xb, rows, 0, head, ld, state);
    launch_cols<4, 64>(xb, rows, head, body, ld, state);
    launch_cols<1, 4>(xb, rows, head + body, cols - head - body, ld, state);
  } else if (cols <= 4) {
    launch_cols<1, 4>(xb, rows, 0, cols, ld, state);
  } else {
    launch_cols<1, 64>(xb, rows, 0, cols, ld, state);
  }
  return launch_status("nqk_absmax_f32");
}
