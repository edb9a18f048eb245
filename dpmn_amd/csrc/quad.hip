// The text regions of whole photos, rectified (utils/quad.py fixes the semantics; main.py --demo_boxes).
// dpmn_quad_crop_u8: a RAGGED batch of RGB uint8 photos (resize.hip's packed layout) and R regions, each a quadrilateral of one photo
// given as the 8 coefficients of PIL's perspective transform -> the R rectified regions (h_r x w_r x 3 bytes each) in the same packed
// layout, byte for byte Image.transform((w, h), PERSPECTIVE, coeffs, BICUBIC):
//   k_quad_crop   block = one 32 x 8 tile of one region (the tile table names it), one thread per output pixel: the pixel's centre
//                 through the transform, then the 4 x 4 bicubic of Geometry.c over the three channels.
// float64 throughout, in the operation order of the restatement: plain * + / (the library is built with -ffp-contract=off, and the
// double division is correctly rounded), the result truncated to a byte.  Neighbouring threads of a tile row read neighbouring source
// pixels (a text region is at most mildly slanted, so a row of 32 pixels touches a few source rows); the 48 bytes of a pixel's taps
// come through L1 / L2 -- no LDS staging.  A few hundred KB per batch: launch-bound work, nothing here is tuned for throughput.
#include "quad_sample.h"

namespace {

constexpr int QUAD_REGION_WORDS = 14;
constexpr int QUAD_TILE_W = 32, QUAD_TILE_H = 8;

// One region as the kernel sees it (include/dpmn_hip.h dpmn_quad_crop_u8: 14 int64 per region).  The numbers are data from the
// caller.  Returns 2 when the region can be computed, 1 when only its output extent is sound (it is written black), 0 when not even
// that is (nothing is written).  The host entry point applies the same test to its copy of the table.
__host__ __device__ inline int quad_region_state(const long long* p, long packed_bytes, long out_bytes) {
  const long long in_off = p[0], H = p[1], W = p[2], out_off = p[3], h = p[4], w = p[5];
  if (!(h >= 1 && h <= RESIZE_MAX_SIDE && w >= 1 && w <= RESIZE_MAX_SIDE && out_off >= 0 && out_off <= out_bytes - h * w * 3)) return 0;
  if (!(H >= 1 && H <= RESIZE_MAX_SIDE && W >= 1 && W <= RESIZE_MAX_SIDE && in_off >= 0 && in_off <= packed_bytes - H * W * 3)) return 1;
  return 2;
}

__global__ void __launch_bounds__(QUAD_TILE_W * QUAD_TILE_H)
k_quad_crop(const unsigned char* __restrict__ packed, long packed_bytes, const long long* __restrict__ regions, int R,
            const int* __restrict__ tiles, unsigned char* __restrict__ out, long out_bytes) {
  const int* t = tiles + (size_t)blockIdx.x * 3;
  const int r = t[0], tile_row = t[1], tile_col = t[2];
  if (r < 0 || r >= R) return;
  const long long* p = regions + (size_t)r * QUAD_REGION_WORDS;
  const int state = quad_region_state(p, packed_bytes, out_bytes);
  if (state == 0) return;
  const int H = (int)p[1], W = (int)p[2], h = (int)p[4], w = (int)p[5];
  // (the tile is data from the caller too: one outside its region writes nothing)
  if (tile_row < 0 || tile_col < 0 || tile_row > (h - 1) / QUAD_TILE_H || tile_col > (w - 1) / QUAD_TILE_W) return;
  const int x = tile_col * QUAD_TILE_W + (int)threadIdx.x, y = tile_row * QUAD_TILE_H + (int)threadIdx.y;
  if (x >= w || y >= h) return;
  unsigned char* dst = out + p[3] + ((size_t)y * w + x) * 3;
  unsigned char px[3] = {0, 0, 0};
  if (state == 2) {
    const double a0 = __longlong_as_double(p[6]), a1 = __longlong_as_double(p[7]), a2 = __longlong_as_double(p[8]);
    const double a3 = __longlong_as_double(p[9]), a4 = __longlong_as_double(p[10]), a5 = __longlong_as_double(p[11]);
    const double a6 = __longlong_as_double(p[12]), a7 = __longlong_as_double(p[13]);
    const double xin = x + 0.5, yin = y + 0.5;
    const double den = a6 * xin + a7 * yin + 1;
    double sx = (a0 * xin + a1 * yin + a2) / den;
    double sy = (a3 * xin + a4 * yin + a5) / den;
    // (a NaN compares false: outside; nothing becomes an integer before this test)
    if (sx >= 0.0 && sx < (double)W && sy >= 0.0 && sy < (double)H) {
      bicubic_sample_u8(packed + p[0], H, W, sx, sy, px);
    }
  }
  dst[0] = px[0];
  dst[1] = px[1];
  dst[2] = px[2];
}

}  // namespace

extern "C" {

int dpmn_quad_crop_u8(const unsigned char* packed, long packed_bytes, const long long* regions, const long long* regions_host, int R,
                      const int* tiles, int n_tiles, unsigned char* out, long out_bytes, dpmn_stream_t stream) {
  if (R == 0) return DPMN_OK;
  DPMN_REQUIRE(packed && regions && regions_host && out, "quad_crop: null pointer");
  DPMN_REQUIRE(R > 0 && n_tiles >= 0 && (tiles || n_tiles == 0), "quad_crop: bad sizes");
  DPMN_REQUIRE(packed_bytes > 0 && out_bytes > 0, "quad_crop: empty buffers");
  int bad = 0;
  for (int r = 0; r < R; ++r) bad += quad_region_state(regions_host + (size_t)r * QUAD_REGION_WORDS, packed_bytes, out_bytes) != 2;
  if (n_tiles > 0) {
    hipLaunchKernelGGL(k_quad_crop, dim3((unsigned)n_tiles), dim3(QUAD_TILE_W, QUAD_TILE_H), 0, as_stream(stream), packed, packed_bytes, regions,
                       R, tiles, out, out_bytes);
    DPMN_CHECK_LAUNCH();
  }
  // the launch has gone out: the sound regions are computed, the others are black
  DPMN_REQUIRE(bad == 0, "quad_crop: a region does not fit the buffers or has a side outside 1 .. 8192 (it is not read and comes out black)");
  return DPMN_OK;
}

}  // extern "C"
