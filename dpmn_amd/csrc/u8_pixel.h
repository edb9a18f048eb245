// What the uint8 image kernels share (resize.hip, tile.hip, display.hip, degrade.hip): the roundings of a float to a byte and the one
// pass of PIL's fixed-point bicubic resample (libImaging/Resample.c).
#pragma once
#include "common.h"

constexpr int RESIZE_THREADS = 256;
constexpr int RESIZE_PRECISION_BITS = 22;         // PIL Resample.c: 32 - 8 - 2
constexpr int RESIZE_MAX_SIDE = 8192;
constexpr int RESIZE_MAX_KSIZE = 2 * 2 * RESIZE_MAX_SIDE + 1;      // 8192 -> 1

__device__ __forceinline__ unsigned char clip8(int acc) { return (unsigned char)min(max(acc >> RESIZE_PRECISION_BITS, 0), 255); }

// ToPILImage on a float tensor: x.mul(255).byte() -- one fp32 multiply, then truncation.  Outside [0, 255] the reference's cast is
// undefined: clamped here (fmaxf drops a NaN: 0).  The formula of display.hip's LR rows.
__device__ __forceinline__ int quant_lr(float x) { return (int)fminf(fmaxf(__fmul_rn(x, 255.0f), 0.0f), 255.0f); }

// save_image: x.mul(255).add_(0.5).clamp_(0, 255).to(uint8) -- two separately rounded fp32 operations, then truncation; fmaxf drops a
// NaN: 0.  A fused multiply-add rounds once and lands on the other side of an integer boundary for inputs next to (k + 0.5) / 255:
// __fmul_rn / __fadd_rn never contract.  The formula of every SR / HR byte.
__device__ __forceinline__ unsigned char quant_sr(float x) {
  return (unsigned char)(int)fminf(fmaxf(__fadd_rn(__fmul_rn(x, 255.0f), 0.5f), 0.0f), 255.0f);
}

// One output byte of a resample pass.  t: the output index's table row [first input index, n taps, k_0 .. k_{ksize-1}], 22 fraction
// bits (utils/resize.py pil_resample_tables); load(i): input sample i as int, called for i in [lo, hi) only -- the table is data from
// the caller, so its first index and tap count are clamped to the valid range.  clip8((2^21 + sum in * k) >> 22) in int32:
// 255 * sum |k| + 2^21 < 2^31 for every size pair up to RESIZE_MAX_SIDE.
template <class Load>
__device__ __forceinline__ unsigned char resample_u8(const int* t, int ksize, int lo, int hi, Load load) {
  const int i0 = min(max(t[0], lo), hi - 1), n = min(min(t[1], ksize), hi - i0);
  int acc = 1 << (RESIZE_PRECISION_BITS - 1);
  for (int k = 0; k < n; ++k) acc += load(i0 + k) * t[2 + k];
  return clip8(acc);
}

// The horizontal pass of an h x w x 3 image to the width out_w, a grid-stride walk of block (x, .) over the h x out_w x 3 bytes of dst.
__device__ __forceinline__ void resample_hor_u8(const unsigned char* src, int h, int w, unsigned char* dst, int out_w, const int* tab, int ksize) {
  const int row_bytes = out_w * 3, tstride = 2 + ksize;
  const long total = (long)h * row_bytes;
  for (long i = (long)blockIdx.x * RESIZE_THREADS + threadIdx.x; i < total; i += (long)gridDim.x * RESIZE_THREADS) {
    const int row = (int)(i / row_bytes), rem = (int)(i - (long)row * row_bytes), x = rem / 3, c = rem - x * 3;
    const unsigned char* p = src + (size_t)row * w * 3 + c;
    dst[i] = resample_u8(tab + (size_t)x * tstride, ksize, 0, w, [p](int j) { return (int)p[(size_t)j * 3]; });
  }
}

// One byte of the vertical pass: column byte `rem` of output row `row` from the h rows of row_bytes bytes at mid.
__device__ __forceinline__ unsigned char resample_ver_u8(const unsigned char* mid, int h, int row_bytes, int rem, int row, const int* tab, int ksize) {
  const unsigned char* p = mid + rem;
  return resample_u8(tab + (size_t)row * (2 + ksize), ksize, 0, h, [p, row_bytes](int j) { return (int)p[(size_t)j * row_bytes]; });
}
