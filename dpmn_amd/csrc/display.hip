// The LR / SR / HR comparison images of an evaluation pass (tripple_display / test_display, interfaces/base.py:275-326 of the
// reference), composed on the device as uint8 so that ONE device-to-host copy serves every PNG of the pass:
//   k_display_triple  per selected image: rows [0, H)   the LR input, ToPILImage's quantisation + PIL's fixed-point bicubic resize
//                                         rows [H, 2H)  the SR output, save_image's quantisation
//                                         rows [2H, 3H) the HR target, save_image's quantisation
// Every stage of the reference is integer arithmetic or a single fp32 operation: the bytes equal the reference's file content.
// Runs a handful of times per evaluation: nothing here is tuned for throughput.
#include "u8_pixel.h"

namespace {

constexpr int DISPLAY_THREADS = 256;
constexpr int DISPLAY_LDS_BYTES = 48 * 1024;      // horizontal-pass intermediate of one row band (uint8, HWC)
constexpr int DISPLAY_MAX_KSIZE = 5;              // bicubic, scale <= 1: ceil(2) * 2 + 1 taps

// Tables (utils/resize.py pil_resample_tables): per output index 2 + ksize int32 = [first input index, n taps, k_0 .. k_{ksize-1}],
// 22 fraction bits.  Block (band, j): output rows [band * band_rows, +band_rows) of all three sections of selected image j.
//   phase 1  the horizontal pass of the input rows this band's vertical pass reads -> LDS (uint8, HWC, at most lds_rows rows)
//   phase 2  the vertical pass from LDS -> section 0
//   phase 3  the SR and HR rows -> sections 1 and 2
// int32 accumulation: 255 * sum |k| * 2^22 < 2^31 for the cubic's sum |k| <= 1.25 + rounding.
__global__ void __launch_bounds__(DISPLAY_THREADS)
k_display_triple(const float* __restrict__ in, long in_bs, long in_cs, const float* __restrict__ sr, long sr_bs, long sr_cs,
                 const float* __restrict__ hr, long hr_bs, long hr_cs, const int* __restrict__ sel, const int* __restrict__ tab_h,
                 const int* __restrict__ tab_v, unsigned char* __restrict__ out, int B, int h, int w, int H, int W, int ksize,
                 int band_rows, int lds_rows) {
  extern __shared__ unsigned char s_hor[];      // (rows, W, 3)
  const int j = blockIdx.y;
  const int r0 = blockIdx.x * band_rows, r1 = min(H, r0 + band_rows);
  const int row_bytes = W * 3, tstride = 2 + ksize;
  unsigned char* o = out + (size_t)j * 3 * H * row_bytes;
  const int b = sel[j];
  if (b < 0 || b >= B) {      // an index outside the batch reads nothing: its triple is black
    for (int i = threadIdx.x; i < (r1 - r0) * row_bytes; i += DISPLAY_THREADS)
      for (int s = 0; s < 3; ++s) o[(size_t)(s * H + r0) * row_bytes + i] = 0;
    return;
  }
  // the bounds grow with the output row: the band reads input rows [y_lo, y_hi)
  const int y_lo = min(max(tab_v[(size_t)r0 * tstride], 0), h - 1);
  int y_hi = min(tab_v[(size_t)(r1 - 1) * tstride] + tab_v[(size_t)(r1 - 1) * tstride + 1], h);
  y_hi = max(min(y_hi, y_lo + lds_rows), y_lo + 1);
  const float* pin = in + (size_t)b * in_bs;
  for (int i = threadIdx.x; i < (y_hi - y_lo) * row_bytes; i += DISPLAY_THREADS) {
    const int row = i / row_bytes, rem = i - row * row_bytes, x = rem / 3, c = rem - x * 3;
    const float* p = pin + (size_t)c * in_cs + (size_t)(y_lo + row) * w;
    s_hor[i] = resample_u8(tab_h + (size_t)x * tstride, ksize, 0, w, [p](int k) { return quant_lr(p[k]); });
  }
  __syncthreads();
  for (int i = threadIdx.x; i < (r1 - r0) * row_bytes; i += DISPLAY_THREADS) {
    const int row = i / row_bytes, rem = i - row * row_bytes;
    const unsigned char* p = s_hor + rem;
    o[(size_t)(r0 + row) * row_bytes + rem] =
        resample_u8(tab_v + (size_t)(r0 + row) * tstride, ksize, y_lo, y_hi, [=](int y) { return (int)p[(y - y_lo) * row_bytes]; });
  }
  const float* psr = sr + (size_t)b * sr_bs;
  const float* phr = hr + (size_t)b * hr_bs;
  for (int i = threadIdx.x; i < (r1 - r0) * row_bytes; i += DISPLAY_THREADS) {
    const int row = i / row_bytes, rem = i - row * row_bytes, x = rem / 3, c = rem - x * 3;
    const size_t px = (size_t)(r0 + row) * W + x;
    o[(size_t)(H + r0 + row) * row_bytes + rem] = quant_sr(psr[(size_t)c * sr_cs + px]);
    o[(size_t)(2 * H + r0 + row) * row_bytes + rem] = quant_sr(phr[(size_t)c * hr_cs + px]);
  }
}

}  // namespace

extern "C" {

int dpmn_display_triple_u8(const float* image_in, long in_batch_stride, long in_chan_stride, const float* image_out, long out_batch_stride,
                           long out_chan_stride, const float* image_target, long tgt_batch_stride, long tgt_chan_stride, const int* sel,
                           int n, const int* tab_h, const int* tab_v, int ksize, unsigned char* out, int B, int h, int w, int H, int W,
                           dpmn_stream_t stream) {
  DPMN_REQUIRE(image_in && image_out && image_target && sel && tab_h && tab_v && out, "display_triple: null pointer");
  DPMN_REQUIRE(B > 0 && n > 0 && n <= 65535 && h > 0 && w > 0 && H > 0 && W > 0, "display_triple: bad sizes");
  DPMN_REQUIRE(h <= H && w <= W, "display_triple: the LR input is only enlarged (h <= H and w <= W)");
  DPMN_REQUIRE(ksize == DISPLAY_MAX_KSIZE, "display_triple: tables of 5 taps expected (bicubic, scale <= 1)");
  DPMN_REQUIRE(in_chan_stride >= (long)h * w && in_batch_stride >= 2 * in_chan_stride + (long)h * w, "display_triple: image_in strides");
  DPMN_REQUIRE(out_chan_stride >= (long)H * W && out_batch_stride >= 2 * out_chan_stride + (long)H * W, "display_triple: image_out strides");
  DPMN_REQUIRE(tgt_chan_stride >= (long)H * W && tgt_batch_stride >= 2 * tgt_chan_stride + (long)H * W, "display_triple: image_target strides");
  // a band of R output rows reads at most ceil(R h / H) + 6 input rows: the windows of its first and last row are <= 2.5 rows
  // beyond their centres, which are (R - 1) h / H apart
  const int row_bytes = W * 3;
  const int cap = DISPLAY_LDS_BYTES / row_bytes;
  DPMN_REQUIRE(cap >= 8 || cap >= h, "display_triple: the image is too wide for the LDS row band");
  int band_rows = H, lds_rows = h;
  if (h > cap) {
    band_rows = (int)(((long)(cap - 6) * H) / h);      // ceil(R h / H) + 6 <= cap
    while (band_rows > 1 && (int)(((long)band_rows * h + H - 1) / H) + 6 > cap) --band_rows;
    lds_rows = cap;
  }
  DPMN_REQUIRE(band_rows >= 1, "display_triple: the image is too wide for the LDS row band");
  const dim3 grid((unsigned)cdiv(H, band_rows), (unsigned)n);
  hipLaunchKernelGGL(k_display_triple, grid, dim3(DISPLAY_THREADS), (size_t)lds_rows * row_bytes, as_stream(stream), image_in,
                     in_batch_stride, in_chan_stride, image_out, out_batch_stride, out_chan_stride, image_target, tgt_batch_stride,
                     tgt_chan_stride, sel, tab_h, tab_v, out, B, h, w, H, W, ksize, band_rows, lds_rows);
  DPMN_CHECK_LAUNCH();
  return DPMN_OK;
}

}  // extern "C"
