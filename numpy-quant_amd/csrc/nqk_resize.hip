// Ragged uint8 images -> resize -> center crop -> table lookup (numpy_quant/images.py ResizeCrop).
//
// The resize is Pillow's 8-bit Image.resize(BILINEAR): two separable passes, horizontal then
// vertical, each an int32 accumulation of uint8 * 22-bit fixed-point weights started at 1 << 21,
// shifted right by 22 and clipped to 0..255.  The weights come from the host (float64 there), so
// nothing here does floating-point arithmetic, and the resized pixel is a uint8 again: the
// 256-entry table of nqk_image_lut finishes the job,
//   out[n][c][y][x] = lut[c][resize_u8(img_n)[top + y][left + x][c]].
// The tap tables already hold only the crop window's coordinates.
//
// One workgroup per (image, tile of output rows).  Phase 1: the horizontal pass for exactly the
// input rows the tile's vertical taps touch, source bytes from global memory, uint8 result to LDS
// as channel planes [c][rows][owp] (owp = ow rounded up to 16; four pixels per lane, one dword
// store per plane).  Phase 2: the vertical pass from LDS, a lane taking a run of one plane row
// (16 bytes per tap for the int8 table, one 16-byte store), the lookup in the LDS copy of the table.
#include <vector>
#include "nqk_common.h"

namespace nqk {
namespace {

constexpr int kBits = 22;
constexpr int32_t kRound = 1 << (kBits - 1);
constexpr int kTileRows = 16;              // output rows per workgroup at most
constexpr int64_t kMidSoft = 32 << 10;     // intermediate bytes per workgroup aimed at (4+ workgroups per CU)
constexpr int64_t kMidHard = NQK_RESIZE_LDS_BYTES;  // ... and taken when even one output row needs more

__device__ __forceinline__ uint32_t clip8(int32_t acc) {
  const int32_t v = acc >> kBits;
  return (uint32_t)(v < 0 ? 0 : v > 255 ? 255 : v);
}

// C: the channel count, or 0 for the runtime value c (1..4).  RUN: pixels per lane in phase 2
// (16 with 16-byte LDS reads and stores for a 1-byte table, else 4).
template <typename T, int C, int RUN>
__global__ __launch_bounds__(kThreads) void k_resize_lut(const uint8_t* __restrict__ pixels,
                                                         const nqk_resize_image* __restrict__ desc,
                                                         const int32_t* __restrict__ taps, const T* __restrict__ lut,
                                                         T* __restrict__ out, int c, int oh, int ow, int tile_rows,
                                                         int tiles) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int cc = C ? C : c;
  T* s_lut = reinterpret_cast<T*>(smem);
  uint8_t* s_mid = smem + (size_t)cc * 256 * sizeof(T);  // a multiple of 256 bytes
  const int tid = threadIdx.x;
  const int ni = blockIdx.x / tiles, tile = blockIdx.x - ni * tiles;
  const int y0 = tile * tile_rows;
  const int ny = oh - y0 < tile_rows ? oh - y0 : tile_rows;
  const int owp = (ow + 15) & ~15;

  const nqk_resize_image d = desc[ni];
  const int32_t* xt = taps + d.xtab;
  const int32_t* yt = taps + d.ytab;
  const int kx = xt[0], ky = yt[0];
  const int32_t* xb = xt + 2;
  const int32_t* xw = xb + 2 * (int64_t)ow;
  const int32_t* yb = yt + 2;
  const int32_t* yw = yb + 2 * (int64_t)oh;

  // the input rows this tile's vertical taps touch (uniform over the workgroup)
  int row_lo = INT32_MAX, row_hi = 0;
  for (int j = 0; j < ny; ++j) {
    const int first = yb[2 * (y0 + j)], nt = yb[2 * (y0 + j) + 1];
    row_lo = first < row_lo ? first : row_lo;
    row_hi = first + nt > row_hi ? first + nt : row_hi;
  }
  const int nrows = row_hi > row_lo ? row_hi - row_lo : 0;

  for (int i = tid; i < cc * 256; i += kThreads) s_lut[i] = lut[i];

  // phase 1: horizontal pass, rows row_lo .. row_hi, output columns 0 .. owp (zero past ow)
  const uint8_t* img = pixels + d.offset;
  const int groups = owp >> 2;
  for (int it = tid; it < nrows * groups; it += kThreads) {
    const int r = it / groups, xg = it - r * groups;
    const uint8_t* row = img + (int64_t)(row_lo + r) * d.w * cc;
    uint32_t packed[4] = {0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int x = xg * 4 + j;
      if (x < ow) {
        const int first = xb[2 * x], nt = xb[2 * x + 1];
        const int32_t* wt = xw + (int64_t)x * kx;
        const uint8_t* s = row + (int64_t)first * cc;
        int32_t acc[4] = {kRound, kRound, kRound, kRound};
        for (int k = 0; k < nt; ++k) {
          const int32_t wk = wt[k];
#pragma unroll
          for (int ch = 0; ch < 4; ++ch)
            if (ch < cc) acc[ch] += (int32_t)s[k * cc + ch] * wk;
        }
#pragma unroll
        for (int ch = 0; ch < 4; ++ch) packed[ch] |= clip8(acc[ch]) << (8 * j);
      }
    }
#pragma unroll
    for (int ch = 0; ch < 4; ++ch)
      if (ch < cc) *reinterpret_cast<uint32_t*>(s_mid + (size_t)(ch * nrows + r) * owp + xg * 4) = packed[ch];
  }
  __syncthreads();

  // phase 2: vertical pass from LDS, table lookup, store
  const int runs = owp / RUN;
  for (int it = tid; it < ny * cc * runs; it += kThreads) {
    const int xr = it % runs, t = it / runs;
    const int ch = t % cc, y = y0 + t / cc;
    const int first = yb[2 * y] - row_lo, nt = yb[2 * y + 1];
    const int32_t* wt = yw + (int64_t)y * ky;
    const uint8_t* m = s_mid + (size_t)(ch * nrows + first) * owp + xr * RUN;
    int32_t acc[RUN];
#pragma unroll
    for (int i = 0; i < RUN; ++i) acc[i] = kRound;
    for (int k = 0; k < nt; ++k) {
      const int32_t wk = wt[k];
      uint32_t v[RUN / 4];
      if constexpr (RUN == 16) {
        const uint4 q = *reinterpret_cast<const uint4*>(m + (size_t)k * owp);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
      } else {
        v[0] = *reinterpret_cast<const uint32_t*>(m + (size_t)k * owp);
      }
#pragma unroll
      for (int i = 0; i < RUN; ++i) acc[i] += (int32_t)((v[i >> 2] >> ((i & 3) * 8)) & 255u) * wk;
    }
    const int x0 = xr * RUN;
    const int npix = ow - x0 < RUN ? ow - x0 : RUN;  // <= 0 for a run in the padding only
    T* dst = out + (((int64_t)ni * cc + ch) * oh + y) * ow + x0;
    const T* tab = s_lut + ch * 256;
    if constexpr (RUN == 16 && sizeof(T) == 1) {
      // decided from the address: outputs are offset views, and rows of ow % 16 != 0 shift it
      if (npix == RUN && (((uintptr_t)dst) & 15) == 0) {
        uint32_t o[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          uint32_t word = 0;
#pragma unroll
          for (int b = 0; b < 4; ++b) word |= (uint32_t)(uint8_t)tab[clip8(acc[q * 4 + b])] << (8 * b);
          o[q] = word;
        }
        *reinterpret_cast<uint4*>(dst) = make_uint4(o[0], o[1], o[2], o[3]);
        continue;
      }
    }
#pragma unroll
    for (int i = 0; i < RUN; ++i)
      if (i < npix) dst[i] = tab[clip8(acc[i])];
  }
}

struct Table {  // a validated tap table
  int32_t index;
  int64_t count, in_size;
};

// Everything of a tap table that the kernel turns into an address or adds up: 0 or fail().
int check_table(const int32_t* taps, int64_t words, int32_t index, int64_t count, int64_t in_size, std::vector<Table>& seen) {
  for (const Table& t : seen)
    if (t.index == index && t.count == count && t.in_size == in_size) return 0;
  if (index < 0 || (int64_t)index + 2 > words) return fail("nqk_image_resize_lut: tap table index outside the blob");
  const int64_t ksize = taps[index], cnt = taps[index + 1];
  if (ksize < 1 || ksize > NQK_RESIZE_MAX_TAPS) return fail("nqk_image_resize_lut: tap table ksize outside 1..NQK_RESIZE_MAX_TAPS");
  if (cnt != count) return fail("nqk_image_resize_lut: tap table count is not the output size");
  if ((int64_t)index + 2 + 2 * count + count * ksize > words) return fail("nqk_image_resize_lut: tap table extends past the blob");
  const int32_t* bounds = taps + index + 2;
  const int32_t* weights = bounds + 2 * count;
  for (int64_t i = 0; i < count; ++i) {
    const int64_t first = bounds[2 * i], nt = bounds[2 * i + 1];
    if (first < 0 || nt < 0 || nt > ksize || first + nt > in_size)
      return fail("nqk_image_resize_lut: taps outside the image (first >= 0, n <= ksize, first + n <= size)");
    int64_t sum = 0;
    for (int64_t k = 0; k < nt; ++k) {
      const int64_t w = weights[i * ksize + k];
      sum += w < 0 ? -w : w;
    }
    if (255 * sum + kRound >= (int64_t)1 << 31) return fail("nqk_image_resize_lut: tap weights overflow the int32 accumulator");
  }
  seen.push_back({index, count, in_size});
  return 0;
}

// the most input rows a tile of tile_rows output rows touches
int64_t tile_span(const int32_t* taps, int32_t index, int64_t oh, int64_t tile_rows) {
  const int32_t* bounds = taps + index + 2;
  int64_t span = 0;
  for (int64_t y0 = 0; y0 < oh; y0 += tile_rows) {
    int64_t lo = INT64_MAX, hi = 0;
    for (int64_t y = y0; y < oh && y < y0 + tile_rows; ++y) {
      const int64_t first = bounds[2 * y], nt = bounds[2 * y + 1];
      lo = first < lo ? first : lo;
      hi = first + nt > hi ? first + nt : hi;
    }
    if (hi - lo > span) span = hi - lo;
  }
  return span;
}

template <typename T>
void launch(int64_t grid, size_t lds, const uint8_t* pixels, const nqk_resize_image* desc,
            const int32_t* taps, const void* lut, void* out, int c, int oh, int ow, int tile_rows, int tiles) {
  if constexpr (sizeof(T) == 1) {
    if (c == 3)
      hipLaunchKernelGGL((k_resize_lut<T, 3, 16>), dim3((unsigned)grid), dim3(kThreads), lds, stream(), pixels, desc, taps,
                         (const T*)lut, (T*)out, c, oh, ow, tile_rows, tiles);
    else
      hipLaunchKernelGGL((k_resize_lut<T, 0, 16>), dim3((unsigned)grid), dim3(kThreads), lds, stream(), pixels, desc, taps,
                         (const T*)lut, (T*)out, c, oh, ow, tile_rows, tiles);
  } else {
    hipLaunchKernelGGL((k_resize_lut<T, 0, 4>), dim3((unsigned)grid), dim3(kThreads), lds, stream(), pixels, desc, taps,
                       (const T*)lut, (T*)out, c, oh, ow, tile_rows, tiles);
  }
}

}  // namespace
}  // namespace nqk

using namespace nqk;

extern "C" int nqk_image_resize_lut(const uint8_t* pixels, int64_t pixel_bytes, const void* meta_dev, const void* meta_host,
                                    int64_t meta_bytes, const void* lut, int lut_dtype, void* out, int64_t n, int64_t c,
                                    int64_t oh, int64_t ow) {
  if (!pixels || !meta_dev || !meta_host || !lut || !out) return fail("nqk_image_resize_lut: null pointer");
  if (c < 1 || c > 4) return fail("nqk_image_resize_lut: 1 to 4 channels");
  if (n <= 0 || oh <= 0 || ow <= 0 || pixel_bytes <= 0) return fail("nqk_image_resize_lut: non-positive dimension");
  if (lut_dtype < NQK_I8 || lut_dtype > NQK_F32) return fail("nqk_image_resize_lut: unknown table dtype");
  if (oh > (1 << 20) || ow > (1 << 20) || n > (1 << 24)) return fail("nqk_image_resize_lut: image batch too large");
  if ((((uintptr_t)meta_dev) | ((uintptr_t)meta_host)) & 7) return fail("nqk_image_resize_lut: descriptors not 8-byte aligned");
  const int64_t desc_bytes = n * (int64_t)sizeof(nqk_resize_image);
  if (meta_bytes < desc_bytes || ((meta_bytes - desc_bytes) & 3)) return fail("nqk_image_resize_lut: descriptor bytes do not hold n descriptors and int32 taps");
  const int64_t words = (meta_bytes - desc_bytes) / 4;
  if (words > INT32_MAX) return fail("nqk_image_resize_lut: tap blob too large");
  const nqk_resize_image* desc = static_cast<const nqk_resize_image*>(meta_host);
  const int32_t* taps = reinterpret_cast<const int32_t*>(static_cast<const uint8_t*>(meta_host) + desc_bytes);

  std::vector<Table> xs, ys;
  for (int64_t i = 0; i < n; ++i) {
    const nqk_resize_image& d = desc[i];
    if (d.h < 1 || d.w < 1) return fail("nqk_image_resize_lut: non-positive image size");
    if (d.offset < 0 || d.offset > pixel_bytes || (int64_t)d.h * d.w > (pixel_bytes - d.offset) / c)
      return fail("nqk_image_resize_lut: image outside the pixel buffer");
    if (check_table(taps, words, d.xtab, ow, d.w, xs) || check_table(taps, words, d.ytab, oh, d.h, ys)) return -1;
  }

  // tile rows: the largest tile whose intermediate rows fit the budget aimed at, else the hard one
  const int64_t owp = (ow + 15) & ~(int64_t)15;
  int64_t tile_rows = 0, rows = 0;
  for (const int64_t budget : {kMidSoft, kMidHard}) {
    for (int64_t tr = kTileRows; tr >= 1 && !tile_rows; tr >>= 1) {
      rows = 0;
      for (const Table& t : ys) {
        const int64_t s = tile_span(taps, t.index, oh, tr);
        rows = s > rows ? s : rows;
      }
      if (rows * owp * c <= budget) tile_rows = tr;
    }
    if (tile_rows) break;
  }
  if (!tile_rows) return fail("nqk_image_resize_lut: one output row's intermediate rows exceed NQK_RESIZE_LDS_BYTES");
  const int64_t tiles = (oh + tile_rows - 1) / tile_rows;
  if (n * tiles > INT32_MAX) return fail("nqk_image_resize_lut: image batch too large");
  const size_t esize = lut_dtype == NQK_F32 ? 4 : (size_t)1 << (lut_dtype - NQK_I8);
  const size_t lds = (size_t)c * 256 * esize + (size_t)(rows * owp * c);

  const nqk_resize_image* desc_dev = static_cast<const nqk_resize_image*>(meta_dev);
  const int32_t* taps_dev = reinterpret_cast<const int32_t*>(static_cast<const uint8_t*>(meta_dev) + desc_bytes);
  if (lut_dtype == NQK_F32) {
    launch<float>(n * tiles, lds, pixels, desc_dev, taps_dev, lut, out, (int)c, (int)oh, (int)ow, (int)tile_rows, (int)tiles);
  } else {
    NQK_INT_DISPATCH(lut_dtype, T, launch<T>(n * tiles, lds, pixels, desc_dev, taps_dev, lut, out, (int)c, (int)oh,
                                             (int)ow, (int)tile_rows, (int)tiles));
  }
  return launch_status("nqk_image_resize_lut");
}
