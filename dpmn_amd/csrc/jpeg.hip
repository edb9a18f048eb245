// JPEG artefacts for the synthesised LR training images (dataset/dataset.py:559 JPEG_compress, the stage the reference left commented
// out at :1298-1300): a uniform batch of B RGB uint8 images (B, h, w, 3) after a baseline JPEG of the image's own quality was written
// and read back, without the file in between -- Huffman coding is lossless, so the bytes are those of the lossy stages alone.  The
// semantics are those of utils/jpeg.py jpeg_roundtrip_u8, which restates libjpeg with PIL's defaults (4:2:0, standard tables scaled by
// jpeg_set_quality(q, force_baseline), islow DCT both ways, fancy upsampling); everything is int32, no floating point, no MFMA.
//   k_jpeg_mcu      grid (MCU, image), one wavefront per 16 x 16 MCU.  Lane l owns the 2 x 2 pixels (2 (l >> 3), 2 (l & 7)) of the MCU:
//                   RGB -> YCbCr, the four Y samples and the downsampled Cb / Cr sample (bias 1, 2 by column parity), level-shifted,
//                   into six 8 x 8 blocks in LDS.  Pixels right of the image are its last column's, Y rows below it its last row's,
//                   and chroma rows below it its last CHROMA row's (libjpeg pads the rows after downsampling).  Lanes 0 .. 47 then own
//                   one row of one block (forward row pass), then one column: forward column pass, quantise (|x| + 4 q) / (8 q) with the
//                   sign restored, dequantise, inverse column pass -- all on the eight values in registers -- and last one row again:
//                   inverse row pass, + 128, clamp, one 8-byte store into the workspace planes.  The two tables of the image's quality
//                   are built by the 64 lanes (one entry of each per lane) from the constant base tables.
//   k_jpeg_finish   grid (pixels, image), one thread per output pixel: Y and the triangle-filtered chroma of the workspace planes
//                   (neighbouring MCUs' chroma, hence the second launch), YCbCr -> RGB, three bytes.  Images of quality <= 0 are
//                   copied here and skipped in the first launch.
// LDS: a block's rows are 9 dwords apart, blocks 72: lane i of a row pass reads dword 9 i + j, lane i of a column pass 9 r + i + const
// (72 = 8 mod 32) -- both walk 32 different banks within a 32-lane half.  The stores of the first phase are 2-way (column stride 2).
// Workspace per image: the Y plane (Hp x Wp, sides rounded up to 16) and the Cb, Cr planes (Hp / 2 x Wp / 2), bytes.
#include "common.h"

namespace {

constexpr int JPEG_MAX_SIDE = 1024;
constexpr int JP_PITCH = 9, JP_BLOCK = 8 * JP_PITCH;
constexpr int JP_FIN_THREADS = 256;

__constant__ unsigned char c_jpeg_base[2][64] = {
    {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};

// jfdctint.c / jidctint.c: CONST_BITS 13, PASS1_BITS 2
constexpr int JP_CB = 13, JP_P1 = 2;
constexpr int F_0_298 = 2446, F_0_390 = 3196, F_0_541 = 4433, F_0_765 = 6270, F_0_899 = 7373, F_1_175 = 9633;
constexpr int F_1_501 = 12299, F_1_847 = 15137, F_1_961 = 16069, F_2_053 = 16819, F_2_562 = 20995, F_3_072 = 25172;

__device__ __forceinline__ int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// one pass of jpeg_fdct_islow over d[0..7], in place
template <bool FIRST>
__device__ __forceinline__ void fdct8(int (&d)[8]) {
  const int t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6];
  const int t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  constexpr int SH = FIRST ? JP_CB - JP_P1 : JP_CB + JP_P1;
  d[0] = FIRST ? (t10 + t11) << JP_P1 : descale(t10 + t11, JP_P1);
  d[4] = FIRST ? (t10 - t11) << JP_P1 : descale(t10 - t11, JP_P1);
  const int y1 = (t12 + t13) * F_0_541;
  d[2] = descale(y1 + t13 * F_0_765, SH);
  d[6] = descale(y1 + t12 * (-F_1_847), SH);
  const int z5 = (t4 + t6 + t5 + t7) * F_1_175;
  const int z1 = (t4 + t7) * (-F_0_899), z2 = (t5 + t6) * (-F_2_562);
  const int z3 = (t4 + t6) * (-F_1_961) + z5, z4 = (t5 + t7) * (-F_0_390) + z5;
  d[7] = descale(t4 * F_0_298 + z1 + z3, SH);
  d[5] = descale(t5 * F_2_053 + z2 + z4, SH);
  d[3] = descale(t6 * F_3_072 + z2 + z3, SH);
  d[1] = descale(t7 * F_1_501 + z1 + z4, SH);
}

// one pass of jpeg_idct_islow over d[0..7], in place
template <bool FIRST>
__device__ __forceinline__ void idct8(int (&d)[8]) {
  const int y1 = (d[2] + d[6]) * F_0_541;
  const int e2 = y1 + d[6] * (-F_1_847), e3 = y1 + d[2] * F_0_765;
  const int e0 = (d[0] + d[4]) << JP_CB, e1 = (d[0] - d[4]) << JP_CB;
  const int t10 = e0 + e3, t13 = e0 - e3, t11 = e1 + e2, t12 = e1 - e2;
  int t0 = d[7], t1 = d[5], t2 = d[3], t3 = d[1];
  const int z5 = (t0 + t2 + t1 + t3) * F_1_175;
  const int z1 = (t0 + t3) * (-F_0_899), z2 = (t1 + t2) * (-F_2_562);
  const int z3 = (t0 + t2) * (-F_1_961) + z5, z4 = (t1 + t3) * (-F_0_390) + z5;
  t0 = t0 * F_0_298 + z1 + z3;
  t1 = t1 * F_2_053 + z2 + z4;
  t2 = t2 * F_3_072 + z2 + z3;
  t3 = t3 * F_1_501 + z1 + z4;
  constexpr int SH = FIRST ? JP_CB - JP_P1 : JP_CB + JP_P1 + 3;
  d[0] = descale(t10 + t3, SH); d[7] = descale(t10 - t3, SH);
  d[1] = descale(t11 + t2, SH); d[6] = descale(t11 - t2, SH);
  d[2] = descale(t12 + t1, SH); d[5] = descale(t12 - t1, SH);
  d[3] = descale(t13 + t0, SH); d[4] = descale(t13 - t0, SH);
}

__device__ __forceinline__ int clamp8(int v) { return min(max(v, 0), 255); }

// jccolor.c: FIX(x) = round(x * 2^16)
__device__ __forceinline__ void rgb_ycc(const unsigned char* p, int& y, int& cb, int& cr) {
  const int r = p[0], g = p[1], b = p[2];
  y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
  cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;
  cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
}

struct Planes {
  int Wp, Wc;                   // row lengths of the Y plane and of a chroma plane
  size_t y, cb, cr;             // byte offsets of image b's planes in the workspace
};
__device__ __forceinline__ Planes planes_of(int b, int h, int w) {
  const int Hp = (h + 15) & ~15, Wp = (w + 15) & ~15;
  Planes p;
  p.Wp = Wp; p.Wc = Wp >> 1;
  const size_t ysz = (size_t)Hp * Wp;
  p.y = (size_t)b * (ysz + (ysz >> 1));
  p.cb = p.y + ysz;
  p.cr = p.cb + (ysz >> 2);
  return p;
}

__global__ void __launch_bounds__(64)
k_jpeg_mcu(const unsigned char* __restrict__ in, const int* __restrict__ quality, int h, int w, int mcus_x, unsigned char* __restrict__ ws) {
  __shared__ int blk[6 * JP_BLOCK];
  __shared__ int qt[2][64];
  const int b = blockIdx.y, l = threadIdx.x;
  int q = quality[b];
  if (q <= 0) return;                                  // left alone: k_jpeg_finish copies it
  q = min(q, 100);
  {
    const int scale = q < 50 ? 5000 / q : 200 - 2 * q;               // jpeg_quality_scaling
    qt[0][l] = min(max(((int)c_jpeg_base[0][l] * scale + 50) / 100, 1), 255);
    qt[1][l] = min(max(((int)c_jpeg_base[1][l] * scale + 50) / 100, 1), 255);
  }
  const int my = blockIdx.x / mcus_x, mx = blockIdx.x - my * mcus_x;
  // ---- the lane's 2 x 2 pixels -> 4 Y samples, 1 Cb, 1 Cr
  {
    const int qy = l >> 3, qx = l & 7;
    const int ch = (h + 1) >> 1;
    const int x0 = min(mx * 16 + 2 * qx, w - 1), x1 = min(mx * 16 + 2 * qx + 1, w - 1);
    const int yr0 = min(my * 16 + 2 * qy, h - 1), yr1 = min(my * 16 + 2 * qy + 1, h - 1);       // the Y samples' rows
    const int cy = min(my * 8 + qy, ch - 1);                                                    // the chroma sample's row ...
    const int cr0 = 2 * cy, cr1 = min(2 * cy + 1, h - 1);                                       // ... and the rows it averages
    const unsigned char* img = in + (size_t)b * h * w * 3;
    int* yb = blk + ((qy >> 2) * 2 + (qx >> 2)) * JP_BLOCK + ((2 * qy) & 7) * JP_PITCH + ((2 * qx) & 7);
    const bool same = yr0 == cr0;             // false only below an image of even height (then yr0 == yr1 == h - 1, cr0 == h - 2)
    int y, cb, cr, scb = 0, scr = 0;
    rgb_ycc(img + ((size_t)yr0 * w + x0) * 3, y, cb, cr);
    yb[0] = y - 128; scb += cb; scr += cr;
    rgb_ycc(img + ((size_t)yr0 * w + x1) * 3, y, cb, cr);
    yb[1] = y - 128; scb += cb; scr += cr;
    rgb_ycc(img + ((size_t)yr1 * w + x0) * 3, y, cb, cr);
    yb[JP_PITCH] = y - 128; scb += cb; scr += cr;
    rgb_ycc(img + ((size_t)yr1 * w + x1) * 3, y, cb, cr);
    yb[JP_PITCH + 1] = y - 128; scb += cb; scr += cr;
    if (!same) {
      scb = 0; scr = 0;
      rgb_ycc(img + ((size_t)cr0 * w + x0) * 3, y, cb, cr); scb += cb; scr += cr;
      rgb_ycc(img + ((size_t)cr0 * w + x1) * 3, y, cb, cr); scb += cb; scr += cr;
      rgb_ycc(img + ((size_t)cr1 * w + x0) * 3, y, cb, cr); scb += cb; scr += cr;
      rgb_ycc(img + ((size_t)cr1 * w + x1) * 3, y, cb, cr); scb += cb; scr += cr;
    }
    const int bias = 1 + (qx & 1);
    blk[4 * JP_BLOCK + qy * JP_PITCH + qx] = ((scb + bias) >> 2) - 128;
    blk[5 * JP_BLOCK + qy * JP_PITCH + qx] = ((scr + bias) >> 2) - 128;
  }
  __syncthreads();
  const int bi = l >> 3, k = l & 7;                    // block, and the row or column of it this lane owns (lanes 0 .. 47)
  int d[8];
  if (l < 48) {                                        // forward, rows
    int* p = blk + bi * JP_BLOCK + k * JP_PITCH;
#pragma unroll
    for (int j = 0; j < 8; ++j) d[j] = p[j];
    fdct8<true>(d);
#pragma unroll
    for (int j = 0; j < 8; ++j) p[j] = d[j];
  }
  __syncthreads();
  if (l < 48) {                                        // forward columns, quantise, dequantise, inverse columns
    int* p = blk + bi * JP_BLOCK + k;
    const int* t = qt[bi >= 4] + k;
#pragma unroll
    for (int j = 0; j < 8; ++j) d[j] = p[j * JP_PITCH];
    fdct8<false>(d);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int qv = t[j * 8], q8 = qv << 3;
      const int a = (abs(d[j]) + (q8 >> 1)) / q8;
      d[j] = (d[j] < 0 ? -a : a) * qv;
    }
    idct8<true>(d);
#pragma unroll
    for (int j = 0; j < 8; ++j) p[j * JP_PITCH] = d[j];
  }
  __syncthreads();
  if (l < 48) {                                        // inverse rows -> the workspace planes
    const int* p = blk + bi * JP_BLOCK + k * JP_PITCH;
#pragma unroll
    for (int j = 0; j < 8; ++j) d[j] = p[j];
    idct8<false>(d);
    unsigned lo = 0, hi = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      lo |= (unsigned)clamp8(d[j] + 128) << (8 * j);
      hi |= (unsigned)clamp8(d[j + 4] + 128) << (8 * j);
    }
    const Planes pl = planes_of(b, h, w);
    size_t o;
    if (bi < 4) o = pl.y + (size_t)(my * 16 + (bi >> 1) * 8 + k) * pl.Wp + mx * 16 + (bi & 1) * 8;
    else o = (bi == 4 ? pl.cb : pl.cr) + (size_t)(my * 8 + k) * pl.Wc + mx * 8;
    *reinterpret_cast<uint2*>(ws + o) = make_uint2(lo, hi);          // o is a multiple of 8: plane sizes, row lengths and columns are
  }
}

// h2v2_fancy_upsample at output pixel (y, x) of a chroma plane with ch x cw real samples (cw > 2)
__device__ __forceinline__ int fancy_at(const unsigned char* __restrict__ c, int Wc, int ch, int cw, int y, int x) {
  const int cy = y >> 1, cx = x >> 1;
  const int oy = (y & 1) ? min(cy + 1, ch - 1) : max(cy - 1, 0);
  const unsigned char *r0 = c + (size_t)cy * Wc, *r1 = c + (size_t)oy * Wc;
  const int s = 3 * r0[cx] + r1[cx];
  if (x & 1) return cx == cw - 1 ? (4 * s + 7) >> 4 : (3 * s + 3 * r0[cx + 1] + r1[cx + 1] + 7) >> 4;
  return cx == 0 ? (4 * s + 8) >> 4 : (3 * s + 3 * r0[cx - 1] + r1[cx - 1] + 8) >> 4;
}

__global__ void __launch_bounds__(JP_FIN_THREADS)
k_jpeg_finish(const unsigned char* in, const int* __restrict__ quality, int h, int w, const unsigned char* __restrict__ ws, unsigned char* out) {
  const int b = blockIdx.y, px = blockIdx.x * JP_FIN_THREADS + threadIdx.x;
  if (px >= h * w) return;
  const size_t o = ((size_t)b * h * w + px) * 3;
  if (quality[b] <= 0) {
    if (in != out) { out[o] = in[o]; out[o + 1] = in[o + 1]; out[o + 2] = in[o + 2]; }
    return;
  }
  const int y = px / w, x = px - y * w;
  const Planes pl = planes_of(b, h, w);
  const int ch = (h + 1) >> 1, cw = (w + 1) >> 1;
  const int Y = ws[pl.y + (size_t)y * pl.Wp + x];
  int cb, cr;
  if (cw > 2) {
    cb = fancy_at(ws + pl.cb, pl.Wc, ch, cw, y, x);
    cr = fancy_at(ws + pl.cr, pl.Wc, ch, cw, y, x);
  } else {                                             // jinit_upsampler: no fancy upsampling for downsampled_width <= 2
    cb = ws[pl.cb + (size_t)(y >> 1) * pl.Wc + (x >> 1)];
    cr = ws[pl.cr + (size_t)(y >> 1) * pl.Wc + (x >> 1)];
  }
  cb -= 128; cr -= 128;
  // jdcolor.c: FIX(1.40200), FIX(0.34414), FIX(0.71414), FIX(1.77200)
  out[o] = (unsigned char)clamp8(Y + ((91881 * cr + 32768) >> 16));
  out[o + 1] = (unsigned char)clamp8(Y + ((-22554 * cb + 32768 - 46802 * cr) >> 16));
  out[o + 2] = (unsigned char)clamp8(Y + ((116130 * cb + 32768) >> 16));
}

}  // namespace

extern "C" {

size_t dpmn_jpeg_roundtrip_workspace_bytes(int B, int h, int w) {
  if (B <= 0 || h <= 0 || w <= 0 || h > JPEG_MAX_SIDE || w > JPEG_MAX_SIDE) return 0;
  const size_t ysz = (size_t)((h + 15) & ~15) * (size_t)((w + 15) & ~15);
  return (size_t)B * (ysz + (ysz >> 1));
}

int dpmn_jpeg_roundtrip_u8(const unsigned char* in, unsigned char* out, const int* quality, int B, int h, int w, void* workspace,
                           size_t workspace_bytes, dpmn_stream_t stream) {
  DPMN_REQUIRE(in && out && quality && workspace, "jpeg_roundtrip: null pointer");
  DPMN_REQUIRE(B > 0 && B <= 65535 && h >= 1 && h <= JPEG_MAX_SIDE && w >= 1 && w <= JPEG_MAX_SIDE,
               "jpeg_roundtrip: bad sizes (1 <= B <= 65535, sides 1 .. 1024)");
  DPMN_REQUIRE(workspace_bytes >= dpmn_jpeg_roundtrip_workspace_bytes(B, h, w), "jpeg_roundtrip: workspace too small");
  DPMN_REQUIRE(((uintptr_t)workspace & 7) == 0, "jpeg_roundtrip: the workspace must be 8-byte aligned");
  const int mcus_x = (w + 15) / 16, mcus_y = (h + 15) / 16;
  hipLaunchKernelGGL(k_jpeg_mcu, dim3((unsigned)(mcus_x * mcus_y), (unsigned)B), dim3(64), 0, as_stream(stream), in, quality, h, w, mcus_x,
                     (unsigned char*)workspace);
  DPMN_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_jpeg_finish, dim3((unsigned)((h * w + JP_FIN_THREADS - 1) / JP_FIN_THREADS), (unsigned)B), dim3(JP_FIN_THREADS), 0,
                     as_stream(stream), in, quality, h, w, (const unsigned char*)workspace, out);
  DPMN_CHECK_LAUNCH();
  return DPMN_OK;
}

}  // extern "C"
