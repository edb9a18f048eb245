// The super-resolved text regions pasted back into their enlarged photo (utils/paste.py fixes the semantics; main.py --demo_paste): the
// inverse of quad.hip.  dpmn_paste_regions_u8: one H2 x W2 x 3 uint8 photo, modified IN PLACE, the SR images in resize.hip's packed
// layout and R regions, each the 8 coefficients of PIL's perspective transform from the photo to one SR image plus a feather width ->
// per region, in list order, Image.paste(SR.transform((W2, H2), PERSPECTIVE, coeffs, BICUBIC), mask) with the mask of utils/paste.py:
//   k_paste_regions   block = one 32 x 8 tile of the PHOTO that at least one region's bounding box meets (the tile table names it and
//                     its slice of the flat region list), one thread per pixel: it walks the tile's regions in list order -- the
//                     pixel's centre through the transform, inside the SR rectangle? then the 4 x 4 bicubic of Geometry.c
//                     (quad_sample.h), the feather mask and PIL's integer blend -- keeps the three running bytes in registers and
//                     writes them once.
// No byte of the photo has two owners, and a thread reads its pixel before it writes it: in place is safe and the result does not
// depend on the schedule.  float64 throughout, in the operation order of the restatement: plain * + / (the library is built with
// -ffp-contract=off, and the double division is correctly rounded).  The work is proportional to the area the boxes cover, not to the
// photo's; the taps come through L1 / L2 as in quad.hip.
#include "paste_common.h"

namespace {

constexpr int PASTE_REGION_WORDS = 12;      // include/dpmn_hip.h dpmn_paste_regions_u8: 12 int64 per region

__global__ void __launch_bounds__(PASTE_TILE_W * PASTE_TILE_H)
k_paste_regions(unsigned char* __restrict__ photo, int H2, int W2, const unsigned char* __restrict__ sr, long sr_bytes,
                const long long* __restrict__ regions, int R, const int* __restrict__ tiles, const int* __restrict__ list, int n_list) {
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
    const long long* p = regions + (size_t)r * PASTE_REGION_WORDS;
    if (!paste_region_ok(p, sr_bytes)) continue;
    const int h_s = (int)p[1], w_s = (int)p[2];
    const double feather = __longlong_as_double(p[3]);
    const double a0 = __longlong_as_double(p[4]), a1 = __longlong_as_double(p[5]), a2 = __longlong_as_double(p[6]);
    const double a3 = __longlong_as_double(p[7]), a4 = __longlong_as_double(p[8]), a5 = __longlong_as_double(p[9]);
    const double a6 = __longlong_as_double(p[10]), a7 = __longlong_as_double(p[11]);
    const double den = a6 * xin + a7 * yin + 1;
    const double sx = (a0 * xin + a1 * yin + a2) / den;
    const double sy = (a3 * xin + a4 * yin + a5) / den;
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

int dpmn_paste_regions_u8(unsigned char* photo, int H2, int W2, const unsigned char* sr, long sr_bytes, const long long* regions,
                          const long long* regions_host, int R, const int* tiles, int n_tiles, const int* list, int n_list,
                          dpmn_stream_t stream) {
  if (R == 0 || n_tiles == 0) return DPMN_OK;
  DPMN_REQUIRE(photo && sr && regions && regions_host && tiles && list, "paste_regions: null pointer");
  DPMN_REQUIRE(R > 0 && n_tiles > 0 && n_list > 0, "paste_regions: bad sizes");
  DPMN_REQUIRE(H2 >= 1 && H2 <= RESIZE_MAX_SIDE && W2 >= 1 && W2 <= RESIZE_MAX_SIDE, "paste_regions: a side of the photo outside 1 .. 8192");
  DPMN_REQUIRE(sr_bytes > 0, "paste_regions: empty SR buffer");
  {
    // the two buffers must not overlap: the photo is written while the SR images are read
    const unsigned char* lo = photo;
    const unsigned char* hi = photo + (size_t)H2 * W2 * 3;
    DPMN_REQUIRE(sr + sr_bytes <= lo || sr >= hi, "paste_regions: the photo and the SR buffer overlap");
  }
  for (int r = 0; r < R; ++r)
    DPMN_REQUIRE(paste_region_ok(regions_host + (size_t)r * PASTE_REGION_WORDS, sr_bytes),
                 "paste_regions: a region's SR image does not fit the buffer or has a side outside 1 .. 8192 (nothing is pasted)");
  hipLaunchKernelGGL(k_paste_regions, dim3((unsigned)n_tiles), dim3(PASTE_TILE_W, PASTE_TILE_H), 0, as_stream(stream), photo, H2, W2, sr,
                     sr_bytes, regions, R, tiles, list, n_list);
  DPMN_CHECK_LAUNCH();
  return DPMN_OK;
}

}  // extern "C"
