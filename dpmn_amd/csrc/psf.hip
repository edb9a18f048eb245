// A random point-spread function per image on a RAGGED batch (main.py --psf_blur: camera shake, defocus, an elongated Gaussian), and
// the cutblur column copy as a launch of its own.  B RGB uint8 images of B sizes in the packed layout of dpmn_resize_ragged_u8; every
// image comes out at its own size in the same layout.  The semantics are those of utils/psf.py:
//   k_psf_blur   per byte (2^15 + sum over the image's taps of q * in[fold101(y + dy), fold101(x + dx)]) >> 16.  The taps (dy, dx, q)
//                are 16-bit integer weights, q > 0 with sum 2^16, quantised once on the host (psf_taps): integer arithmetic only, no
//                atomics, so the bytes are those of psf_blur_u8 in every compute mode and on every run.  The sum is at most
//                255 * 2^16 + 2^15 < 2^31: int32 never wraps.
//   k_cutblur    the columns >= cut_x (side 1) or < cut_x (side 2) of the LR buffer become the HR image's (utils/psf.py cutblur_u8).
// k_psf_blur: one block = one 32 x 32 tile of one image (host-built tile table, as degrade.hip).  The tile grown by the IMAGE's own
// radius R <= 10 is staged into LDS once, folded at the image's borders on load (BORDER_REFLECT_101, as often as needed), as ONE
// 32-bit word R | G << 8 | B << 16 per pixel: at most 52 x 52 words.  The image's taps sit in LDS as (offset in the staged window, q).
// A thread owns column lx of rows ly, ly + 8, ..: per tap one tap read (one address per wave: a broadcast) and one pixel word read
// (32 consecutive words per half wave: conflict-free on the 32 banks of ds_read_b32), three int32 multiply-adds.  Only the non-zero taps are
// walked -- a motion PSF has a few K of K^2.  An identity PSF is R = 0 with one tap of 2^16: the same path copies the bytes.
// About a megabyte per batch and two blocks per CU: the call lasts as long as its slowest block's tap walk (DESIGN.md (f) has the
// numbers); nothing here is tuned for throughput.
#include "u8_pixel.h"

namespace {

constexpr int PSF_THREADS = 256;
constexpr int PSF_TILE = 32;
constexpr int PSF_MAX_R = 10;
constexpr int PSF_SIDE = PSF_TILE + 2 * PSF_MAX_R;                   // 52
constexpr int PSF_MAX_TAPS = (2 * PSF_MAX_R + 1) * (2 * PSF_MAX_R + 1);      // 441
constexpr int PSF_ROWS = PSF_THREADS / PSF_TILE;                     // 8 rows of the tile per sweep
constexpr int PSF_ONE = 1 << 16;

// BORDER_REFLECT_101, folded as often as needed
__device__ __forceinline__ int psf_fold101(int i, int n) {
  if (n == 1) return 0;
  const int p = 2 * (n - 1);
  i %= p;
  if (i < 0) i += p;
  return i < n ? i : p - i;
}

__device__ __forceinline__ bool image_ok(long long off, long long h, long long w, long packed_bytes) {
  return h >= 1 && h <= RESIZE_MAX_SIDE && w >= 1 && w <= RESIZE_MAX_SIDE && off >= 0 && off <= packed_bytes - h * w * 3;
}

// items: 4 int64 per image [byte offset, h, w, first tile]; psf: 3 int32 per image [first tap, taps, R]; taps: 3 int32 per tap.  All of
// it is data from the caller: an image, a tile or a PSF that does not fit is not read and not written, a tap outside R is skipped.
__global__ void __launch_bounds__(PSF_THREADS)
k_psf_blur(const unsigned char* __restrict__ packed, long packed_bytes, const long long* __restrict__ items, const int* __restrict__ tiles,
           int n_tiles, const int* __restrict__ psf, const int* __restrict__ taps, int n_taps, int B, unsigned char* __restrict__ out) {
  __shared__ unsigned int pix[PSF_SIDE * PSF_SIDE];
  __shared__ int2 tap[PSF_MAX_TAPS];
  const int tile = blockIdx.x, b = tiles[tile * 3], ty = tiles[tile * 3 + 1], tx = tiles[tile * 3 + 2];
  if (b < 0 || b >= B || ty < 0 || tx < 0) return;
  const long long* it = items + (size_t)b * 4;
  const long long off = it[0], hh = it[1], ww = it[2], ft = it[3];
  if (!image_ok(off, hh, ww, packed_bytes) || ft < 0 || ft >= n_tiles) return;
  const int h = (int)hh, w = (int)ww, tiles_x = (w + PSF_TILE - 1) / PSF_TILE;
  const int ty0 = ty * PSF_TILE, tx0 = tx * PSF_TILE;
  if (ty0 >= h || tx0 >= w || (long long)tile != ft + (long long)ty * tiles_x + tx) return;
  const int first = psf[b * 3], count = psf[b * 3 + 1], R = psf[b * 3 + 2];
  if (first < 0 || count < 1 || count > PSF_MAX_TAPS || first > n_taps - count || R < 0 || R > PSF_MAX_R) return;

  // ---- the image's taps: (offset of the tap in the staged window, q)
  for (int t = threadIdx.x; t < count; t += PSF_THREADS) {
    const int* p = taps + (size_t)(first + t) * 3;
    const int dy = p[0], dx = p[1], q = p[2];
    const bool ok = dy >= -R && dy <= R && dx >= -R && dx <= R && q > 0 && q <= PSF_ONE;
    tap[t] = ok ? make_int2(dy * PSF_SIDE + dx, q) : make_int2(0, 0);
  }
  // ---- the tile grown by R, folded into the image: window row i = image row fold(ty0 - R + i)
  const int th = min(PSF_TILE, h - ty0), tw = min(PSF_TILE, w - tx0), nh = th + 2 * R, nw = tw + 2 * R;
  const unsigned char* src = packed + off;
  for (int e = threadIdx.x; e < nh * nw; e += PSF_THREADS) {
    const int i = e / nw, j = e - i * nw;
    const unsigned char* p = src + ((size_t)psf_fold101(ty0 - R + i, h) * w + psf_fold101(tx0 - R + j, w)) * 3;
    pix[i * PSF_SIDE + j] = (unsigned)p[0] | ((unsigned)p[1] << 8) | ((unsigned)p[2] << 16);
  }
  __syncthreads();
  // ---- every pixel of the tile: the non-zero taps only
  const int lx = threadIdx.x % PSF_TILE, ly0 = threadIdx.x / PSF_TILE;
  if (lx >= tw) return;
  unsigned char* dst = out + off;
  for (int ly = ly0; ly < th; ly += PSF_ROWS) {
    const unsigned int* c = pix + (ly + R) * PSF_SIDE + lx + R;
    int ar = PSF_ONE >> 1, ag = PSF_ONE >> 1, ab = PSF_ONE >> 1;
    for (int t = 0; t < count; ++t) {
      const int2 k = tap[t];
      const unsigned v = c[k.x];
      ar += k.y * (int)(v & 255u);
      ag += k.y * (int)((v >> 8) & 255u);
      ab += k.y * (int)(v >> 16);
    }
    unsigned char* o = dst + ((size_t)(ty0 + ly) * w + tx0 + lx) * 3;
    o[0] = (unsigned char)(ar >> 16);
    o[1] = (unsigned char)(ag >> 16);
    o[2] = (unsigned char)(ab >> 16);
  }
}

// block (x, b): a grid-stride walk over the h x w x 3 bytes of image b; cuts: 5 int64 per image [byte offset, h, w, cut_x, cut_side]
__global__ void __launch_bounds__(PSF_THREADS)
k_cutblur(const unsigned char* __restrict__ hr, long packed_bytes, const long long* __restrict__ cuts, unsigned char* __restrict__ low) {
  const long long* p = cuts + (size_t)blockIdx.y * 5;
  const long long off = p[0], h = p[1], w = p[2], cut_x = p[3], side = p[4];
  if ((side != 1 && side != 2) || !image_ok(off, h, w, packed_bytes)) return;
  const int row_bytes = (int)w * 3;
  const long total = (long)h * row_bytes;
  for (long i = (long)blockIdx.x * PSF_THREADS + threadIdx.x; i < total; i += (long)gridDim.x * PSF_THREADS) {
    const int x = (int)(i % row_bytes) / 3;
    if (side == 1 ? x >= cut_x : x < cut_x) low[off + i] = hr[off + i];
  }
}

}  // namespace

extern "C" {

int dpmn_psf_blur_ragged_u8(const unsigned char* packed_in, long packed_bytes, const long long* items, const int* tiles, int n_tiles,
                            const int* psf, const int* taps, int n_taps, int B, unsigned char* packed_out, dpmn_stream_t stream) {
  DPMN_REQUIRE(packed_in && items && tiles && psf && taps && packed_out, "psf_blur_ragged: null pointer");
  DPMN_REQUIRE(packed_in != packed_out, "psf_blur_ragged: in place is not supported (tiles read their neighbours' input)");
  DPMN_REQUIRE(B > 0 && B <= 65535 && n_tiles >= B && n_taps >= B && packed_bytes > 0,
               "psf_blur_ragged: bad sizes (1 <= B <= 65535, a tile and a tap per image at least)");
  hipLaunchKernelGGL(k_psf_blur, dim3((unsigned)n_tiles), dim3(PSF_THREADS), 0, as_stream(stream), packed_in, packed_bytes, items, tiles,
                     n_tiles, psf, taps, n_taps, B, packed_out);
  DPMN_CHECK_LAUNCH();
  return DPMN_OK;
}

int dpmn_cutblur_ragged_u8(const unsigned char* packed_hr, long packed_bytes, const long long* cuts, int B, int max_pixels,
                           unsigned char* packed_low, dpmn_stream_t stream) {
  DPMN_REQUIRE(packed_hr && cuts && packed_low, "cutblur_ragged: null pointer");
  DPMN_REQUIRE(packed_hr != packed_low, "cutblur_ragged: the LR buffer must not be the HR buffer");
  DPMN_REQUIRE(B > 0 && B <= 65535 && max_pixels > 0 && packed_bytes > 0, "cutblur_ragged: bad sizes (1 <= B <= 65535)");
  const long blocks = ((long)max_pixels * 3 + PSF_THREADS - 1) / PSF_THREADS;
  hipLaunchKernelGGL(k_cutblur, dim3((unsigned)(blocks < 256 ? blocks : 256), (unsigned)B), dim3(PSF_THREADS), 0, as_stream(stream),
                     packed_hr, packed_bytes, cuts, packed_low);
  DPMN_CHECK_LAUNCH();
  return DPMN_OK;
}

}  // extern "C"
