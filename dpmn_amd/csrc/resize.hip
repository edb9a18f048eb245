// PIL's fixed-point bicubic resize (libImaging/Resample.c, what Image.resize(..., BICUBIC) runs on uint8) for a RAGGED batch: B RGB
// images of B different sizes, packed back to back in one buffer, each resized to one common H x W -- enlarging or shrinking, per axis.
//   k_resize_hor   horizontal pass of every input row -> the ragged intermediate (h_b x W x 3 bytes per image), ROUNDED AND CLIPPED to
//                  uint8 as in PIL
//   k_resize_ver   vertical pass of the intermediate -> out (B, H, W, 3)
// Per output index a table row [first input index, n taps, k_0 ..] with 22 fraction bits (utils/resize.py pil_resample_tables, built
// on the host in float64 in PIL's operation order); a pixel is clip8((2^21 + sum in * k) >> 22) in int32 (255 * sum |k| + 2^21 < 2^31
// for every size pair up to 8192).  Integer arithmetic only: the bytes equal PIL's and do not depend on the compute mode.  An axis
// whose sizes are equal goes through its identity table like any other.  The tap count is 2 * ceil(2 * scale) + 1 when shrinking, so
// neither pass keeps a band in LDS: two launches and a global intermediate serve every size pair with one code path.  A few hundred
// KB per batch: launch-bound work, nothing here is tuned for throughput.
// k_quantize_sr    save_image's quantisation of an NCHW float batch -> (B, H, W, 3) uint8, the bytes of the SR image files.
#include "u8_pixel.h"

namespace {

constexpr int RESIZE_ITEM_WORDS = 8;

// One image of the batch as the kernels see it (include/dpmn_hip.h dpmn_resize_ragged_u8: 8 int64 per image).
struct Item {
  long in_off, mid_off;
  const int *tab_h, *tab_v;
  int h, w, ksize_h, ksize_v;
  bool ok;
};

// The item is data from the caller: an image whose numbers do not fit the buffers is not read (its output is black).
__device__ __forceinline__ Item load_item(const long long* __restrict__ items, int b, long packed_bytes, long mid_bytes, int W) {
  const long long* p = items + (size_t)b * RESIZE_ITEM_WORDS;
  Item it;
  it.in_off = p[0]; it.mid_off = p[3];
  const long long h = p[1], w = p[2], kh = p[5], kv = p[7];
  it.tab_h = reinterpret_cast<const int*>(p[4]);
  it.tab_v = reinterpret_cast<const int*>(p[6]);
  it.ok = h >= 1 && h <= RESIZE_MAX_SIDE && w >= 1 && w <= RESIZE_MAX_SIDE && kh >= 1 && kh <= RESIZE_MAX_KSIZE && kv >= 1 &&
          kv <= RESIZE_MAX_KSIZE && it.tab_h && it.tab_v && it.in_off >= 0 && it.in_off <= packed_bytes - h * w * 3 && it.mid_off >= 0 &&
          it.mid_off <= mid_bytes - h * W * 3;
  it.h = (int)h; it.w = (int)w; it.ksize_h = (int)kh; it.ksize_v = (int)kv;
  return it;
}

// block (x, b): a grid-stride walk over the h_b x W x 3 intermediate bytes of image b
__global__ void __launch_bounds__(RESIZE_THREADS)
k_resize_hor(const unsigned char* __restrict__ packed, long packed_bytes, const long long* __restrict__ items, unsigned char* __restrict__ mid,
             long mid_bytes, int W) {
  const Item it = load_item(items, blockIdx.y, packed_bytes, mid_bytes, W);
  if (!it.ok) return;
  resample_hor_u8(packed + it.in_off, it.h, it.w, mid + it.mid_off, W, it.tab_h, it.ksize_h);
}

// block (x, b): RESIZE_THREADS of the H x W x 3 output bytes of image b
__global__ void __launch_bounds__(RESIZE_THREADS)
k_resize_ver(const unsigned char* __restrict__ mid, long mid_bytes, long packed_bytes, const long long* __restrict__ items,
             unsigned char* __restrict__ out, int H, int W) {
  const int row_bytes = W * 3;
  const int i = blockIdx.x * RESIZE_THREADS + threadIdx.x;
  if (i >= H * row_bytes) return;
  unsigned char* o = out + (size_t)blockIdx.y * H * row_bytes;
  const Item it = load_item(items, blockIdx.y, packed_bytes, mid_bytes, W);
  if (!it.ok) {
    o[i] = 0;
    return;
  }
  const int row = i / row_bytes;
  o[i] = resample_ver_u8(mid + it.mid_off, it.h, row_bytes, i - row * row_bytes, row, it.tab_v, it.ksize_v);
}

__global__ void __launch_bounds__(RESIZE_THREADS)
k_quantize_sr(const float* __restrict__ x, long bs, long cs, unsigned char* __restrict__ out, int HW, long total) {
  const long i = (long)blockIdx.x * RESIZE_THREADS + threadIdx.x;      // index into (B, H, W, 3)
  if (i >= total) return;
  const long px = i / 3;
  const int c = (int)(i - px * 3);
  const long b = px / HW, r = px - b * HW;
  out[i] = quant_sr(x[(size_t)b * bs + (size_t)c * cs + r]);
}

}  // namespace

extern "C" {

size_t dpmn_resize_ragged_workspace_bytes(long sum_h, int W) {
  return sum_h > 0 && W > 0 ? (size_t)sum_h * W * 3 : 0;
}

int dpmn_resize_ragged_u8(const unsigned char* packed, long packed_bytes, const long long* items, int B, int max_h, unsigned char* out, int H,
                          int W, unsigned char* workspace, size_t workspace_bytes, dpmn_stream_t stream) {
  DPMN_REQUIRE(packed && items && out && workspace, "resize_ragged: null pointer");
  DPMN_REQUIRE(B > 0 && B <= 65535 && H > 0 && W > 0 && H <= RESIZE_MAX_SIDE && W <= RESIZE_MAX_SIDE, "resize_ragged: bad sizes (B <= 65535, H and W <= 8192)");
  DPMN_REQUIRE(max_h > 0 && max_h <= RESIZE_MAX_SIDE, "resize_ragged: max_h outside 1 .. 8192");
  DPMN_REQUIRE(packed_bytes > 0 && workspace_bytes > 0 && workspace_bytes <= (size_t)1 << 62, "resize_ragged: empty buffers");
  const long row_bytes = (long)W * 3;
  const long hor_blocks = (max_h * row_bytes + RESIZE_THREADS - 1) / RESIZE_THREADS;      // the tallest image; the others stride less
  const unsigned gx = (unsigned)(hor_blocks < 256 ? hor_blocks : 256);
  hipLaunchKernelGGL(k_resize_hor, dim3(gx, (unsigned)B), dim3(RESIZE_THREADS), 0, as_stream(stream), packed, packed_bytes, items, workspace,
                     (long)workspace_bytes, W);
  DPMN_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_resize_ver, dim3((unsigned)((H * row_bytes + RESIZE_THREADS - 1) / RESIZE_THREADS), (unsigned)B), dim3(RESIZE_THREADS), 0,
                     as_stream(stream), workspace, (long)workspace_bytes, packed_bytes, items, out, H, W);
  DPMN_CHECK_LAUNCH();
  return DPMN_OK;
}

int dpmn_quantize_sr_u8(const float* x, long batch_stride, long chan_stride, unsigned char* out, int B, int H, int W, dpmn_stream_t stream) {
  DPMN_REQUIRE(x && out && B > 0 && H > 0 && W > 0, "quantize_sr: bad arguments");
  DPMN_REQUIRE(chan_stride >= (long)H * W && (B == 1 || batch_stride >= 2 * chan_stride + (long)H * W), "quantize_sr: strides");
  const long total = (long)B * H * W * 3;
  hipLaunchKernelGGL(k_quantize_sr, dim3((unsigned)((total + RESIZE_THREADS - 1) / RESIZE_THREADS)), dim3(RESIZE_THREADS), 0, as_stream(stream),
                     x, batch_stride, chan_stride, out, H * W, total);
  DPMN_CHECK_LAUNCH();
  return DPMN_OK;
}

}  // extern "C"
