// Quadrilaterals and polygons pasted back into their enlarged photo in ONE list (utils/paste_poly.py fixes the semantics; main.py
// --demo_paste_polygons): paste.hip's launch with a second kind of region.  dpmn_paste_mixed_u8: one H2 x W2 x 3 uint8 photo, modified
// IN PLACE, the SR images in resize.hip's packed layout, R regions and a strip table.  A perspective region is paste.hip's: 8
// coefficients from the photo to its SR image.  A polygon region names a slice of the strip table; a strip is a four-cornered piece of
// the photo, the SR columns it covers and its bounding box, and the pixel's source position is the INVERSE of the strip's bilinear map:
//   k_paste_mixed     block = one 32 x 8 tile of the PHOTO that at least one region's box meets, one thread per pixel: it walks the
//                     tile's regions in list order.  Perspective: paste.hip's arithmetic.  Polygon: it walks the region's strips,
//                     skips a strip whose box does not hold the pixel (integers, before any float64 work), solves the strip's
//                     quadratic for the rest and stops at the first strip with 0 <= u < 1, 0 <= v < 1.  Then for either kind the
//                     inside test, feather mask, bicubic sample and blend of paste_common.h.  The three running bytes stay in
//                     registers and are written once.
// No byte of the photo has two owners, and a thread reads its pixel before it writes it: in place is safe and the result does not
// depend on the schedule.  float64 throughout, in the operation order of the restatement: plain * + - /, and sqrt (the library is built
// with -ffp-contract=off and without fast-math: the double division and square root are the device library's correctly rounded ones).
#include "paste_common.h"

namespace {

constexpr int MIXED_REGION_WORDS = 13;      // include/dpmn_hip.h dpmn_paste_mixed_u8: 13 int64 per region
constexpr int MIXED_STRIP_WORDS = 14;       //                                          14 int64 per strip
constexpr int MIXED_MAX_STRIPS = 31;        // utils.poly.MAX_POLY_SIDE - 1
constexpr long long KIND_PERSPECTIVE = 0, KIND_POLYGON = 1;

// One region as the kernel sees it: paste_common.h's test of its SR image, a known kind, and for a polygon a slice of 1 .. 31 strips
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
