// The two roundings to a byte that the uint8 image kernels share (resize.hip, tile.hip).
#pragma once
#include "common.h"

constexpr int RESIZE_THREADS = 256;
constexpr int RESIZE_PRECISION_BITS = 22;         // PIL Resample.c: 32 - 8 - 2
constexpr int RESIZE_MAX_SIDE = 8192;
constexpr int RESIZE_MAX_KSIZE = 2 * 2 * RESIZE_MAX_SIDE + 1;      // 8192 -> 1

__device__ __forceinline__ unsigned char clip8(int acc) { return (unsigned char)min(max(acc >> RESIZE_PRECISION_BITS, 0), 255); }

// save_image: x.mul(255).add_(0.5).clamp_(0, 255).to(uint8) -- two separately rounded fp32 operations (__fmul_rn / __fadd_rn never
// contract), then truncation; fmaxf drops a NaN: 0.  The formula of display.hip's SR / HR rows.
__device__ __forceinline__ unsigned char quant_sr(float x) {
  return (unsigned char)(int)fminf(fmaxf(__fadd_rn(__fmul_rn(x, 255.0f), 0.5f), 0.0f), 255.0f);
}
