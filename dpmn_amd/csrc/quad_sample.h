// What the warping kernels share (quad.hip, poly.hip and paste_poly.hip): the 4 x 4 bicubic sample
// of PIL's Image.transform (libImaging/Geometry.c) on an RGB uint8 image, float64 in the operation order of utils/quad.py's restatement.
#pragma once
#include "u8_pixel.h"

// Geometry.c BICUBIC: the cubic through four values at the fraction d, in its operation order
__device__ __forceinline__ double cubic(double v1, double v2, double v3, double v4, double d) {
  const double p1 = v2;
  const double p2 = -v1 + v3;
  const double p3 = 2 * (v1 - v2) + v3 - v4;
  const double p4 = -v1 + v2 - v3 + v4;
  return p1 + d * (p2 + d * (p3 + d * p4));
}

// The three bytes of an H x W x 3 image at the source position (sx, sy), which the caller has found inside 0 <= sx < W, 0 <= sy < H
// (before the -0.5 shift that is applied here): the taps are the columns ix - 1 .. ix + 2, each clipped to the image, and the rows
// iy - 1 .. iy + 2; the byte is the value clamped to 0 .. 255 and truncated.
__device__ __forceinline__ void bicubic_sample_u8(const unsigned char* __restrict__ src, int H, int W, double sx, double sy, unsigned char px[3]) {
  sx -= 0.5;
  sy -= 0.5;
  const double fx = floor(sx), fy = floor(sy);
  const double dx = sx - fx, dy = sy - fy;
  const int ix = (int)fx, iy = (int)fy;      // -1 .. W - 1, -1 .. H - 1
  const int c0 = min(max(ix - 1, 0), W - 1) * 3, c1 = min(max(ix, 0), W - 1) * 3, c2 = min(max(ix + 1, 0), W - 1) * 3,
            c3 = min(max(ix + 2, 0), W - 1) * 3;
  const size_t row_bytes = (size_t)W * 3;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    double v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int row = iy - 1 + k;
      // the first row is clipped; a later row outside the photo repeats the value of the row before it
      if (k == 0 || (row >= 0 && row < H)) {
        const unsigned char* q = src + (size_t)min(max(row, 0), H - 1) * row_bytes + c;
        v[k] = cubic((double)q[c0], (double)q[c1], (double)q[c2], (double)q[c3], dx);
      } else {
        v[k] = v[k - 1];
      }
    }
    const double val = cubic(v[0], v[1], v[2], v[3], dy);
    px[c] = val <= 0.0 ? 0 : val >= 255.0 ? 255 : (unsigned char)(int)val;
  }
}
