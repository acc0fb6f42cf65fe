// uint8 images -> the model's input tensor by table lookup (numpy_quant/images.py).
//
// Per-channel normalize and quantize are elementwise, so a uint8 pixel of channel c maps to
// one of 256 values: out[n][c][y][x] = lut[c][img[n][y][x][c]] (NHWC input) or
// lut[c][img[n][c][y][x]] (NCHW input).  The table is filled on the host side of the ABI by
// the library's own quantize (or holds the normalized floats), so nothing here does
// floating-point arithmetic and the result is bit-identical to quantize(normalize(img)).
// HBM-bound: 1 B in + sizeof(T) B out per element.
#include "nqk_common.h"

namespace nqk {
namespace {

constexpr int kRun = 16;  // pixels per lane in the int8 NHWC C=3 kernel

// byte k (0..15) of a 16-byte vector held as four dwords
__device__ __forceinline__ uint32_t byte_of(const uint32_t (&v)[12], int k) { return (v[k >> 2] >> ((k & 3) * 8)) & 255u; }

// The hot case: int8 table, NHWC input, 3 channels.  A lane takes a run of 16 pixels of one image
// row: 48 contiguous input bytes as three 16-byte loads, one 16-byte store per channel plane.
// The vector path needs the run's input address and its three output addresses 16-byte aligned
// (decided per run from the addresses: base pointers are offset views, rows of w % 16 != 0 and
// images of h*w % 16 != 0 shift them); row tails and unaligned runs go pixel by pixel.
__global__ void k_image_lut_i8_hwc3(const uint8_t* __restrict__ img, const int8_t* __restrict__ lut,
                                    int8_t* __restrict__ out, int64_t rows, int64_t h, int64_t w) {
  __shared__ int8_t s_lut[3 * 256];
  for (int i = threadIdx.x; i < 3 * 256; i += blockDim.x) s_lut[i] = lut[i];
  __syncthreads();
  const int64_t runs_per_row = (w + kRun - 1) / kRun;
  const int64_t runs = rows * runs_per_row;  // rows = n * h
  const int64_t plane = h * w;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < runs; r += stride) {
    const int64_t row = r / runs_per_row;
    const int64_t x0 = (r - row * runs_per_row) * kRun;
    const int64_t ni = row / h, y = row - ni * h;
    const uint8_t* src = img + (row * w + x0) * 3;
    int8_t* dst = out + (ni * 3 * h + y) * w + x0;  // channel 0; channel c at dst + c * plane
    const int64_t npix = w - x0 < kRun ? w - x0 : kRun;
    const bool aligned = npix == kRun && ((((uintptr_t)src) | ((uintptr_t)dst) | ((uintptr_t)(dst + plane)) |
                                           ((uintptr_t)(dst + 2 * plane))) & 15) == 0;
    if (aligned) {
      uint32_t v[12];
      const uint4* s4 = reinterpret_cast<const uint4*>(src);
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const uint4 t = s4[j];
        v[4 * j] = t.x; v[4 * j + 1] = t.y; v[4 * j + 2] = t.z; v[4 * j + 3] = t.w;
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        uint32_t o[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          uint32_t word = 0;
#pragma unroll
          for (int b = 0; b < 4; ++b) {
            const int p = q * 4 + b;  // pixel of the run; its channel c is input byte 3p + c
            word |= (uint32_t)(uint8_t)s_lut[c * 256 + byte_of(v, 3 * p + c)] << (8 * b);
          }
          o[q] = word;
        }
        *reinterpret_cast<uint4*>(dst + c * plane) = make_uint4(o[0], o[1], o[2], o[3]);
      }
    } else {
      for (int64_t p = 0; p < npix; ++p)
        for (int c = 0; c < 3; ++c) dst[c * plane + p] = s_lut[c * 256 + src[p * 3 + c]];
    }
  }
}

// every other table type, channel count and the NCHW input layout: one output element per thread
template <typename T>
__global__ void k_image_lut(const uint8_t* __restrict__ img, const T* __restrict__ lut, T* __restrict__ out,
                            int64_t total, int64_t plane, int64_t c, int hwc) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const int64_t nc = i / plane, pix = i - nc * plane;  // i = (ni * c + ci) * plane + pix
    const int64_t ni = nc / c, ci = nc - ni * c;
    const int64_t in = hwc ? (ni * plane + pix) * c + ci : i;
    out[i] = lut[ci * 256 + img[in]];
  }
}

}  // namespace
}  // namespace nqk

using namespace nqk;

extern "C" int nqk_image_lut(const uint8_t* img, const void* lut, int lut_dtype, void* out, int64_t n, int64_t h,
                             int64_t w, int64_t c, int layout) {
  if (!img || !lut || !out) return fail("nqk_image_lut: null pointer");
  if (c < 1 || c > 4) return fail("nqk_image_lut: 1 to 4 channels");
  if (n <= 0 || h <= 0 || w <= 0) return fail("nqk_image_lut: non-positive dimension");
  if (layout != NQK_IMG_NHWC && layout != NQK_IMG_NCHW) return fail("nqk_image_lut: unknown layout");
  if (lut_dtype < NQK_I8 || lut_dtype > NQK_F32) return fail("nqk_image_lut: unknown table dtype");
  const int64_t lim = INT64_MAX / 8 / c;  // the output's byte count fits in int64
  if (n > lim / h || n * h > lim / w) return fail("nqk_image_lut: image batch too large");
  const int64_t plane = h * w, total = n * c * plane;
  if (lut_dtype == NQK_I8 && layout == NQK_IMG_NHWC && c == 3) {
    const int64_t runs = n * h * ((w + kRun - 1) / kRun);
    hipLaunchKernelGGL(k_image_lut_i8_hwc3, dim3(grid_for(runs)), dim3(kThreads), 0, stream(), img,
                       (const int8_t*)lut, (int8_t*)out, n * h, h, w);
    return launch_status("nqk_image_lut");
  }
  const unsigned g = grid_for(total);
  const int hwc = layout == NQK_IMG_NHWC;
  if (lut_dtype == NQK_F32) {
    hipLaunchKernelGGL(k_image_lut<float>, dim3(g), dim3(kThreads), 0, stream(), img, (const float*)lut, (float*)out,
                       total, plane, c, hwc);
  } else {
    NQK_INT_DISPATCH(lut_dtype, T, hipLaunchKernelGGL(k_image_lut<T>, dim3(g), dim3(kThreads), 0, stream(), img,
                                                        (const T*)lut, (T*)out, total, plane, c, hwc));
  }
  return launch_status("nqk_image_lut");
}
