// The super-resolved text regions pasted back into their enlarged photo, quadrilaterals and polygons in ONE list (utils/paste.py and
// utils/paste_poly.py fix the semantics; main.py --demo_paste, --demo_paste_polygons): the inverse of quad.hip.  dpmn_paste_mixed_u8:
// one H2 x W2 x 3 uint8 photo, modified IN PLACE, the SR images in resize.hip's packed layout, R regions and a strip table.  A
// perspective region carries the 8 coefficients of PIL's perspective transform from the photo to its SR image: per region, in list
// order, Image.paste(SR.transform((W2, H2), PERSPECTIVE, coeffs, BICUBIC), mask) with the mask of utils/paste.py.  A polygon region
// names a slice of the strip table; a strip is a four-cornered piece of the photo, the SR columns it covers and its bounding box, and
// the pixel's source position is the INVERSE of the strip's bilinear map:
//   k_paste_mixed     block = one 32 x 8 tile of the PHOTO that at least one region's box meets (the tile table names it and its slice
//                     of the flat region list), one thread per pixel: it walks the tile's regions in list order.  Perspective: the
//                     pixel's centre through the transform.  Polygon: it walks the region's strips, skips a strip whose box does not
//                     hold the pixel (integers, before any float64 work), solves the strip's quadratic for the rest and stops at the
//                     first strip with 0 <= u < 1, 0 <= v < 1.  Then for either kind the inside test, feather mask, bicubic sample
//                     (quad_sample.h) and PIL's integer blend.  The three running bytes stay in registers and are written once.
// No byte of the photo has two owners, and a thread reads its pixel before it writes it: in place is safe and the result does not
// depend on the schedule.  float64 throughout, in the operation order of the restatements: plain * + - /, and sqrt (the library is built
// with -ffp-contract=off and without fast-math: the double division and square root are the device library's correctly rounded ones).
// The work is proportional to the area the boxes cover, not to the photo's; the taps come through L1 / L2 as in quad.hip.
#include "quad_sample.h"

namespace {

constexpr int PASTE_TILE_WORDS = 4;
constexpr int PASTE_TILE_W = 32, PASTE_TILE_H = 8;

// The first three words of a region record: [byte offset of the SR image, h_s, w_s].  The numbers are data from the caller: a region
// whose SR image does not fit the packed buffer, or has a side outside 1 .. 8192, is not read.  The host entry point applies the same
// test to its copy of the table and refuses the call.
__host__ __device__ inline bool paste_region_ok(const long long* p, long sr_bytes) {
  const long long off = p[0], h = p[1], w = p[2];
  return h >= 1 && h <= RESIZE_MAX_SIDE && w >= 1 && w <= RESIZE_MAX_SIDE && off >= 0 && off <= sr_bytes - h * w * 3;
}

// A tile record [tile row, tile column, first, count] -> whether it lies in the photo and its slice in the region list (the tile is
// data from the caller: one outside the photo, or whose slice leaves the list, writes nothing)
__device__ __forceinline__ bool paste_tile_ok(const int* t, int H2, int W2, int n_list) {
  const int tile_row = t[0], tile_col = t[1], first = t[2], count = t[3];
  if (tile_row < 0 || tile_col < 0 || tile_row > (H2 - 1) / PASTE_TILE_H || tile_col > (W2 - 1) / PASTE_TILE_W) return false;
  return first >= 0 && count >= 0 && first <= n_list - count;
}

// Image.paste with an L mask on uint8 (libImaging/Paste.c BLEND8 of this Pillow): dst, src, m in 0 .. 255
__device__ __forceinline__ int blend8(int dst, int src, int m) {
  const int t = dst * (255 - m) + src * m + 128;
  return ((t >> 8) + t) >> 8;
}

// One region at one pixel, the source position (sx, sy) given: nothing where it lies outside the h_s x w_s SR image (a NaN compares
// false: outside; nothing becomes an integer before this test), else the feather mask, the bicubic sample and the blend into the three
// running bytes.  Returns whether the pixel was touched.
__device__ __forceinline__ bool paste_sample_blend(const unsigned char* __restrict__ sr_image, int h_s, int w_s, double sx, double sy,
                                                   double feather, int& b0, int& b1, int& b2) {
  if (!(sx >= 0.0 && sx < (double)w_s && sy >= 0.0 && sy < (double)h_s)) return false;
  int m = 255;
  if (feather > 0.0) {
    // the distance of the source position to the nearest edge of the SR rectangle, in SR pixels: 0 <= d, so 0 <= m
    const double d = fmin(fmin(sx, (double)w_s - sx), fmin(sy, (double)h_s - sy));
    const double f = d / feather;
    m = f >= 1.0 ? 255 : (int)floor(f * 255 + 0.5);
    m = min(max(m, 0), 255);
  }
  unsigned char px[3];
  bicubic_sample_u8(sr_image, h_s, w_s, sx, sy, px);
  b0 = blend8(b0, px[0], m);
  b1 = blend8(b1, px[1], m);
  b2 = blend8(b2, px[2], m);
  return true;
}

constexpr int MIXED_REGION_WORDS = 13;      // include/dpmn_hip.h dpmn_paste_mixed_u8: 13 int64 per region
constexpr int MIXED_STRIP_WORDS = 14;       //                                          14 int64 per strip
constexpr int MIXED_MAX_STRIPS = 31;        // utils.poly.MAX_POLY_SIDE - 1
constexpr long long KIND_PERSPECTIVE = 0, KIND_POLYGON = 1;

// One region as the kernel sees it: paste_region_ok's test of its SR image, a known kind, and for a polygon a slice of 1 .. 31 strips
// inside the strip table.  The host entry point applies the same test to its copy of the table and refuses the call.
__host__ __device__ inline bool mixed_region_ok(const long long* p, long sr_bytes, int n_strips) {
  if (!paste_region_ok(p, sr_bytes)) return false;
  if (p[4] == KIND_PERSPECTIVE) return true;
  if (p[4] != KIND_POLYGON) return false;
  const long long first = p[5], count = p[6];
  return count >= 1 && count <= MIXED_MAX_STRIPS && first >= 0 && first <= (long long)n_strips - count;
}

// The inverse of one strip's bilinear map at the point (xin, yin): whether 0 <= u < 1 and 0 <= v < 1, and then the source position in
// the SR image.  q: the strip's 10 float64 as int64 bits [NW, NE, SE, SW as (x, y), c0, c1].  utils/paste_poly.py strip_uv, operation
// for operation; a NaN (no real root, a zero divisor) compares false: the strip does not claim the pixel.
__device__ __forceinline__ bool strip_claims(const long long* __restrict__ q, double xin, double yin, int h_s, double& sx, double& sy) {
  const double nwx = __longlong_as_double(q[0]), nwy = __longlong_as_double(q[1]), nex = __longlong_as_double(q[2]);
  const double ney = __longlong_as_double(q[3]), sex = __longlong_as_double(q[4]), sey = __longlong_as_double(q[5]);
  const double swx = __longlong_as_double(q[6]), swy = __longlong_as_double(q[7]);
  const double ex = nex - nwx, ey = ney - nwy;
  const double fx = swx - nwx, fy = swy - nwy;
  const double gx = sex - swx - nex + nwx, gy = sey - swy - ney + nwy;
  const double hx = xin - nwx, hy = yin - nwy;
  const double A = gx * fy - gy * fx;
  const double B = (hx * gy - hy * gx) + (ex * fy - ey * fx);
  const double C = hx * ey - hy * ex;
  const double disc = B * B - 4 * A * C;
  const double r = sqrt(disc);
  const double v = B >= 0.0 ? (-2 * C) / (B + r) : (-B + r) / (2 * A);
  const double dx = ex + v * gx, dy = ey + v * gy;
  const double nx = hx - v * fx, ny = hy - v * fy;
  const double u = fabs(dx) >= fabs(dy) ? nx / dx : ny / dy;
  if (!(u >= 0.0 && u < 1.0 && v >= 0.0 && v < 1.0)) return false;
  const double c0 = __longlong_as_double(q[8]), c1 = __longlong_as_double(q[9]);
  sx = c0 + u * (c1 - c0);
  sy = v * (double)h_s;
  return true;
}

__global__ void __launch_bounds__(PASTE_TILE_W * PASTE_TILE_H)
k_paste_mixed(unsigned char* __restrict__ photo, int H2, int W2, const unsigned char* __restrict__ sr, long sr_bytes,
              const long long* __restrict__ regions, int R, const long long* __restrict__ strips, int n_strips,
              const int* __restrict__ tiles, const int* __restrict__ list, int n_list) {
  const int* t = tiles + (size_t)blockIdx.x * PASTE_TILE_WORDS;
  if (!paste_tile_ok(t, H2, W2, n_list)) return;
  const int tile_row = t[0], tile_col = t[1], first = t[2], count = t[3];
  const int x = tile_col * PASTE_TILE_W + (int)threadIdx.x, y = tile_row * PASTE_TILE_H + (int)threadIdx.y;
  if (x >= W2 || y >= H2) return;
  unsigned char* dst = photo + ((size_t)y * W2 + x) * 3;
  int b0 = dst[0], b1 = dst[1], b2 = dst[2];
  bool touched = false;
  const double xin = x + 0.5, yin = y + 0.5;
  for (int i = 0; i < count; ++i) {
    const int r = list[first + i];
    if (r < 0 || r >= R) continue;
    const long long* p = regions + (size_t)r * MIXED_REGION_WORDS;
    if (!mixed_region_ok(p, sr_bytes, n_strips)) continue;
    const int h_s = (int)p[1], w_s = (int)p[2];
    const double feather = __longlong_as_double(p[3]);
    double sx, sy;
    if (p[4] == KIND_PERSPECTIVE) {
      const double a0 = __longlong_as_double(p[5]), a1 = __longlong_as_double(p[6]), a2 = __longlong_as_double(p[7]);
      const double a3 = __longlong_as_double(p[8]), a4 = __longlong_as_double(p[9]), a5 = __longlong_as_double(p[10]);
      const double a6 = __longlong_as_double(p[11]), a7 = __longlong_as_double(p[12]);
      const double den = a6 * xin + a7 * yin + 1;
      sx = (a0 * xin + a1 * yin + a2) / den;
      sy = (a3 * xin + a4 * yin + a5) / den;
    } else {
      const long long* q = strips + (size_t)p[5] * MIXED_STRIP_WORDS;
      const int n = (int)p[6];
      bool claimed = false;
      for (int s = 0; s < n && !claimed; ++s, q += MIXED_STRIP_WORDS) {
        // the strip's box [x0, y0, x1, y1): an integer test before any float64 work
        if ((long long)x < q[10] || (long long)y < q[11] || (long long)x >= q[12] || (long long)y >= q[13]) continue;
        claimed = strip_claims(q, xin, yin, h_s, sx, sy);
      }
      if (!claimed) continue;
    }
    touched |= paste_sample_blend(sr + p[0], h_s, w_s, sx, sy, feather, b0, b1, b2);
  }
  if (touched) {
    dst[0] = (unsigned char)b0;
    dst[1] = (unsigned char)b1;
    dst[2] = (unsigned char)b2;
  }
}

}  // namespace

extern "C" {

int dpmn_paste_mixed_u8(unsigned char* photo, int H2, int W2, const unsigned char* sr, long sr_bytes, const long long* regions,
                        const long long* regions_host, int R, const long long* strips, int n_strips, const int* tiles, int n_tiles,
                        const int* list, int n_list, dpmn_stream_t stream) {
  if (R == 0 || n_tiles == 0) return DPMN_OK;
  DPMN_REQUIRE(photo && sr && regions && regions_host && tiles && list, "paste_mixed: null pointer");
  DPMN_REQUIRE(R > 0 && n_tiles > 0 && n_list > 0 && n_strips >= 0, "paste_mixed: bad sizes");
  DPMN_REQUIRE(strips || n_strips == 0, "paste_mixed: strips counted but no strip table");
  DPMN_REQUIRE(H2 >= 1 && H2 <= RESIZE_MAX_SIDE && W2 >= 1 && W2 <= RESIZE_MAX_SIDE, "paste_mixed: a side of the photo outside 1 .. 8192");
  DPMN_REQUIRE(sr_bytes > 0, "paste_mixed: empty SR buffer");
  {
    // the two buffers must not overlap: the photo is written while the SR images are read
    const unsigned char* lo = photo;
    const unsigned char* hi = photo + (size_t)H2 * W2 * 3;
    DPMN_REQUIRE(sr + sr_bytes <= lo || sr >= hi, "paste_mixed: the photo and the SR buffer overlap");
  }
  for (int r = 0; r < R; ++r)
    DPMN_REQUIRE(mixed_region_ok(regions_host + (size_t)r * MIXED_REGION_WORDS, sr_bytes, n_strips),
                 "paste_mixed: a region's SR image does not fit the buffer or has a side outside 1 .. 8192, its kind is unknown or its "
                 "strips leave the strip table (nothing is pasted)");
  hipLaunchKernelGGL(k_paste_mixed, dim3((unsigned)n_tiles), dim3(PASTE_TILE_W, PASTE_TILE_H), 0, as_stream(stream), photo, H2, W2, sr,
                     sr_bytes, regions, R, strips, n_strips, tiles, list, n_list);
  DPMN_CHECK_LAUNCH();
  return DPMN_OK;
}

}  // extern "C"
