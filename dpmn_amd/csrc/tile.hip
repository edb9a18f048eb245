// A wide text line as overlapping windows of the model's LR size (utils/tile.py fixes the semantics; main.py --demo_tile).
// dpmn_resize_windows_u8: a RAGGED batch of RGB uint8 images (resize.hip's packed layout) -> every image resized with PIL's
// fixed-point bicubic to the LR height and ITS OWN width w_line, then cut into lr_h x lr_w windows:
//   k_line_hor   horizontal pass (w -> w_line) of every input row -> the ragged intermediate (h_b x w_line_b x 3 bytes per image),
//                rounded and clipped to uint8 as in PIL
//   k_line_ver   vertical pass (h -> lr_h) of the intermediate -> the ragged lines (lr_h x w_line_b x 3 bytes per image)
//   k_gather     the windows (T, lr_h, lr_w, 3): window t = columns [x0_t, x0_t + lr_w) of the line of image_t
// Every line is resized once; overlapping windows only copy.  The arithmetic is resize.hip's: table rows [first input index, n taps,
// k_0 ..] with 22 fraction bits, a pixel is clip8((2^21 + sum in * k) >> 22) in int32 -- the bytes equal PIL's.  The tables of one
// call come in ONE int32 buffer and the items name them by offset, so a table reference is checked like every other number of an item.
// dpmn_stitch_windows_u8: the SR windows (T, >= 3, H, sr_w) float -> the ragged SR lines (H x scale * w_line_b x 3 bytes per image):
//   k_stitch     one thread per output byte: every window of the image that covers the byte's column is quantised (save_image's rule)
//                and blended with integer weights, (sum wgt * q + W / 2) / W.  Every byte has one owner: plain vector stores.
// A few hundred KB per batch: launch-bound work, nothing here is tuned for throughput.
#include "u8_pixel.h"

namespace {

constexpr int TILE_ITEM_WORDS = 10;
constexpr int TILE_LINE_WORDS = 4;

// One image of the batch as the resize kernels see it (include/dpmn_hip.h dpmn_resize_windows_u8: 10 int64 per image).
struct LineItem {
  long in_off, mid_off, line_off;
  const int *tab_h, *tab_v;
  int h, w, w_line, ksize_h, ksize_v;
  bool ok;
};

// The item is data from the caller: an image whose numbers do not fit the buffers is not read (its windows are black).
__device__ __forceinline__ LineItem load_line_item(const long long* __restrict__ items, int b, long packed_bytes, const int* __restrict__ tables,
                                                   long table_ints, long ws_bytes, int lr_h, int lr_w) {
  const long long* p = items + (size_t)b * TILE_ITEM_WORDS;
  LineItem it;
  const long long in_off = p[0], h = p[1], w = p[2], wl = p[3], mid_off = p[4], line_off = p[5], th = p[6], kh = p[7], tv = p[8], kv = p[9];
  it.ok = h >= 1 && h <= RESIZE_MAX_SIDE && w >= 1 && w <= RESIZE_MAX_SIDE && wl >= lr_w && wl <= RESIZE_MAX_SIDE && kh >= 1 &&
          kh <= RESIZE_MAX_KSIZE && kv >= 1 && kv <= RESIZE_MAX_KSIZE && in_off >= 0 && in_off <= packed_bytes - h * w * 3 &&
          mid_off >= 0 && mid_off <= ws_bytes - h * wl * 3 && line_off >= 0 && line_off <= ws_bytes - (long long)lr_h * wl * 3 &&
          th >= 0 && th <= table_ints - wl * (2 + kh) && tv >= 0 && tv <= table_ints - (long long)lr_h * (2 + kv);
  it.in_off = in_off; it.mid_off = mid_off; it.line_off = line_off;
  it.tab_h = tables + (it.ok ? th : 0);
  it.tab_v = tables + (it.ok ? tv : 0);
  it.h = (int)h; it.w = (int)w; it.w_line = (int)wl; it.ksize_h = (int)kh; it.ksize_v = (int)kv;
  return it;
}

// block (x, b): a grid-stride walk over the h_b x w_line_b x 3 intermediate bytes of image b
__global__ void __launch_bounds__(RESIZE_THREADS)
k_line_hor(const unsigned char* __restrict__ packed, long packed_bytes, const long long* __restrict__ items, const int* __restrict__ tables,
           long table_ints, unsigned char* __restrict__ ws, long ws_bytes, int lr_h, int lr_w) {
  const LineItem it = load_line_item(items, blockIdx.y, packed_bytes, tables, table_ints, ws_bytes, lr_h, lr_w);
  if (!it.ok) return;
  resample_hor_u8(packed + it.in_off, it.h, it.w, ws + it.mid_off, it.w_line, it.tab_h, it.ksize_h);
}

// block (x, b): a grid-stride walk over the lr_h x w_line_b x 3 line bytes of image b
__global__ void __launch_bounds__(RESIZE_THREADS)
k_line_ver(long packed_bytes, const long long* __restrict__ items, const int* __restrict__ tables, long table_ints,
           unsigned char* __restrict__ ws, long ws_bytes, int lr_h, int lr_w) {
  const LineItem it = load_line_item(items, blockIdx.y, packed_bytes, tables, table_ints, ws_bytes, lr_h, lr_w);
  if (!it.ok) return;
  const unsigned char* mid = ws + it.mid_off;
  unsigned char* dst = ws + it.line_off;
  const int row_bytes = it.w_line * 3;
  const long total = (long)lr_h * row_bytes;
  for (long i = (long)blockIdx.x * RESIZE_THREADS + threadIdx.x; i < total; i += (long)gridDim.x * RESIZE_THREADS) {
    const int row = (int)(i / row_bytes);
    dst[i] = resample_ver_u8(mid, it.h, row_bytes, (int)(i - (long)row * row_bytes), row, it.tab_v, it.ksize_v);
  }
}

// one thread per byte of out (T, lr_h, lr_w, 3); a window whose image or start is out of range is black
__global__ void __launch_bounds__(RESIZE_THREADS)
k_gather(long packed_bytes, const long long* __restrict__ items, int B, const int* __restrict__ tables, long table_ints,
         const int* __restrict__ windows, const unsigned char* __restrict__ ws, long ws_bytes, unsigned char* __restrict__ out, int lr_h,
         int lr_w, long total) {
  const long i = (long)blockIdx.x * RESIZE_THREADS + threadIdx.x;
  if (i >= total) return;
  const int win_bytes = lr_h * lr_w * 3;
  const long t = i / win_bytes;
  const int r = (int)(i - t * win_bytes), row = r / (lr_w * 3), rem = r - row * (lr_w * 3);
  const int b = windows[2 * t], x0 = windows[2 * t + 1];
  unsigned char v = 0;
  if (b >= 0 && b < B) {
    const LineItem it = load_line_item(items, b, packed_bytes, tables, table_ints, ws_bytes, lr_h, lr_w);
    if (it.ok && x0 >= 0 && x0 <= it.w_line - lr_w) v = ws[it.line_off + ((size_t)row * it.w_line + x0) * 3 + rem];
  }
  out[i] = v;
}

// block (x, b): a grid-stride walk over the H x scale * w_line_b x 3 bytes of SR line b
__global__ void __launch_bounds__(RESIZE_THREADS)
k_stitch(const float* __restrict__ sr, long bs, long cs, int T, int H, int sr_w, int scale, const long long* __restrict__ lines,
         const int* __restrict__ windows, unsigned char* __restrict__ out, long out_bytes) {
  const long long* p = lines + (size_t)blockIdx.y * TILE_LINE_WORDS;
  const long long out_off = p[0], wl = p[1], first = p[2], n = p[3];
  const int lr_w = sr_w / scale, cap = sr_w / 2;
  // the line is data from the caller: one whose numbers do not fit the buffers is not written
  if (!(wl >= lr_w && wl <= RESIZE_MAX_SIDE && first >= 0 && n >= 1 && first <= (long long)T - n && out_off >= 0 &&
        out_off <= out_bytes - (long long)H * scale * wl * 3))
    return;
  const int b = blockIdx.y, w_line = (int)wl, row_bytes = scale * w_line * 3;
  const int t0 = (int)first, t1 = (int)(first + n) - 1;
  unsigned char* dst = out + out_off;
  const long total = (long)H * row_bytes;
  for (long i = (long)blockIdx.x * RESIZE_THREADS + threadIdx.x; i < total; i += (long)gridDim.x * RESIZE_THREADS) {
    const int row = (int)(i / row_bytes), rem = (int)(i - (long)row * row_bytes), X = rem / 3, c = rem - X * 3;
    long acc = 0, wsum = 0;
    for (int t = t0; t <= t1; ++t) {
      const int x0 = windows[2 * t + 1];
      if (windows[2 * t] != b || x0 < 0 || x0 > w_line - lr_w) continue;
      const int j = X - scale * x0;
      if (j < 0 || j >= sr_w) continue;
      const int wgt = min(min(t == t0 ? cap : j + 1, t == t1 ? cap : sr_w - j), cap);
      acc += (long)wgt * quant_sr(sr[(size_t)t * bs + (size_t)c * cs + (size_t)row * sr_w + j]);
      wsum += wgt;
    }
    dst[i] = wsum > 0 ? (unsigned char)((acc + wsum / 2) / wsum) : 0;
  }
}

unsigned grid_x(long bytes) {
  const long blocks = (bytes + RESIZE_THREADS - 1) / RESIZE_THREADS;
  return (unsigned)(blocks < 1 ? 1 : blocks < 256 ? blocks : 256);
}

}  // namespace

extern "C" {

size_t dpmn_resize_windows_workspace_bytes(long sum_h_w_line, long sum_w_line, int lr_h) {
  return sum_h_w_line > 0 && sum_w_line > 0 && lr_h > 0 ? ((size_t)sum_h_w_line + (size_t)sum_w_line * lr_h) * 3 : 0;
}

int dpmn_resize_windows_u8(const unsigned char* packed, long packed_bytes, const long long* items, int B, const int* tables, long table_ints,
                           const int* windows, int T, long max_mid_bytes, int max_w_line, unsigned char* out, int lr_h, int lr_w,
                           unsigned char* workspace, size_t workspace_bytes, dpmn_stream_t stream) {
  DPMN_REQUIRE(packed && items && tables && windows && out && workspace, "resize_windows: null pointer");
  DPMN_REQUIRE(B > 0 && B <= 65535 && T > 0 && lr_h > 0 && lr_w > 0 && lr_h <= RESIZE_MAX_SIDE && lr_w <= RESIZE_MAX_SIDE,
               "resize_windows: bad sizes (B <= 65535, lr_h and lr_w <= 8192)");
  DPMN_REQUIRE(max_w_line >= lr_w && max_w_line <= RESIZE_MAX_SIDE && max_mid_bytes > 0 &&
               max_mid_bytes <= (long)RESIZE_MAX_SIDE * RESIZE_MAX_SIDE * 3, "resize_windows: max_w_line / max_mid_bytes out of range");
  DPMN_REQUIRE(packed_bytes > 0 && table_ints > 0 && workspace_bytes > 0 && workspace_bytes <= (size_t)1 << 62, "resize_windows: empty buffers");
  const long total = (long)T * lr_h * lr_w * 3;
  DPMN_REQUIRE(total / RESIZE_THREADS < 0x7fffffffL, "resize_windows: too many windows");
  hipLaunchKernelGGL(k_line_hor, dim3(grid_x(max_mid_bytes), (unsigned)B), dim3(RESIZE_THREADS), 0, as_stream(stream), packed, packed_bytes, items,
                     tables, table_ints, workspace, (long)workspace_bytes, lr_h, lr_w);
  DPMN_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_line_ver, dim3(grid_x((long)lr_h * max_w_line * 3), (unsigned)B), dim3(RESIZE_THREADS), 0, as_stream(stream), packed_bytes,
                     items, tables, table_ints, workspace, (long)workspace_bytes, lr_h, lr_w);
  DPMN_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_gather, dim3((unsigned)((total + RESIZE_THREADS - 1) / RESIZE_THREADS)), dim3(RESIZE_THREADS), 0, as_stream(stream),
                     packed_bytes, items, B, tables, table_ints, windows, workspace, (long)workspace_bytes, out, lr_h, lr_w, total);
  DPMN_CHECK_LAUNCH();
  return DPMN_OK;
}

int dpmn_stitch_windows_u8(const float* sr, long batch_stride, long chan_stride, int T, int H, int sr_w, int scale, const long long* lines, int B,
                           const int* windows, int max_w_line, unsigned char* out, long out_bytes, dpmn_stream_t stream) {
  DPMN_REQUIRE(sr && lines && windows && out, "stitch_windows: null pointer");
  DPMN_REQUIRE(B > 0 && B <= 65535 && T > 0 && H > 0 && H <= RESIZE_MAX_SIDE && scale > 0 && sr_w >= 2 * scale && sr_w <= RESIZE_MAX_SIDE &&
               sr_w % scale == 0, "stitch_windows: bad sizes (B <= 65535, H and sr_w <= 8192, sr_w a multiple of scale)");
  DPMN_REQUIRE(chan_stride >= (long)H * sr_w && (T == 1 || batch_stride >= 2 * chan_stride + (long)H * sr_w), "stitch_windows: strides");
  DPMN_REQUIRE(max_w_line >= sr_w / scale && max_w_line <= RESIZE_MAX_SIDE && out_bytes > 0, "stitch_windows: max_w_line / out_bytes out of range");
  hipLaunchKernelGGL(k_stitch, dim3(grid_x((long)H * scale * max_w_line * 3), (unsigned)B), dim3(RESIZE_THREADS), 0, as_stream(stream), sr,
                     batch_stride, chan_stride, T, H, sr_w, scale, lines, windows, out, out_bytes);
  DPMN_CHECK_LAUNCH();
  return DPMN_OK;
}

}  // extern "C"
