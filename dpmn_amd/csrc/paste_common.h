// What the paste kernels share (paste.hip, paste_poly.hip): the tile of the photo, the check of a region's SR image, and what happens to
// a pixel once its source position in the SR image is known -- utils/paste.py's inside test, feather mask, bicubic sample and PIL's
// integer blend, float64 in the operation order of the restatement.
#pragma once
#include "quad_sample.h"

constexpr int PASTE_TILE_WORDS = 4;
constexpr int PASTE_TILE_W = 32, PASTE_TILE_H = 8;

// The first three words of a region record: [byte offset of the SR image, h_s, w_s].  The numbers are data from the caller: a region
// whose SR image does not fit the packed buffer, or has a side outside 1 .. 8192, is not read.  The host entry points apply the same
// test to their copy of the table and refuse the call.
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
