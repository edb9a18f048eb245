// Curved text regions of whole photos, rectified (utils/poly.py fixes the semantics; main.py --demo_polygons).
// dpmn_poly_crop_u8: a RAGGED batch of RGB uint8 photos (resize.hip's packed layout) and R regions, each a polygon of one photo cut
// into at most 31 strips -> the R rectified regions (h_r x w_r x 3 bytes each) in the same packed layout, byte for byte
// Image.transform((w, h), MESH, cells, BICUBIC): a cell is the columns x0 <= x < x1 of the region, mapped from its strip by the 8
// coefficients of PIL's bilinear QUAD transform.
//   k_poly_crop   block = one 32 x 8 tile of one region (the tile table names it), one thread per output pixel: the pixel finds its
//                 cell among the region's bounds (a tile may span several cells), its cell-local centre goes through the bilinear
//                 map, then the 4 x 4 bicubic of Geometry.c over the three channels (quad_sample.h, shared with quad.hip).
// float64 throughout, in the operation order of the restatement: plain * + (the library is built with -ffp-contract=off), the result
// truncated to a byte.  No LDS staging, as in quad.hip: a few hundred KB per batch, launch-bound work, nothing here is tuned for
// throughput.
#include "quad_sample.h"

namespace {

constexpr int POLY_REGION_WORDS = 8, POLY_CELL_WORDS = 10;
constexpr int POLY_MAX_CELLS = 31;      // utils/poly.py MAX_POLY_SIDE - 1
constexpr int POLY_TILE_W = 32, POLY_TILE_H = 8;

// One region as the kernel sees it (include/dpmn_hip.h dpmn_poly_crop_u8: 8 int64 per region, 10 per cell).  The numbers are data
// from the caller.  Returns 2 when the region can be computed, 1 when only its output extent is sound (it is written black), 0 when
// not even that is (nothing is written).  A region is computed only if its photo fits the packed buffer, its cells lie inside the cell
// table and their bounds ascend from 0 to w without a gap.  The host entry point applies the same test to its copies of the tables.
__host__ __device__ inline int poly_region_state(const long long* p, const long long* cells, long n_cells, long packed_bytes, long out_bytes) {
  const long long in_off = p[0], H = p[1], W = p[2], out_off = p[3], h = p[4], w = p[5], first = p[6], n = p[7];
  if (!(h >= 1 && h <= RESIZE_MAX_SIDE && w >= 1 && w <= RESIZE_MAX_SIDE && out_off >= 0 && out_off <= out_bytes - h * w * 3)) return 0;
  if (!(H >= 1 && H <= RESIZE_MAX_SIDE && W >= 1 && W <= RESIZE_MAX_SIDE && in_off >= 0 && in_off <= packed_bytes - H * W * 3)) return 1;
  if (!(n >= 1 && n <= POLY_MAX_CELLS && first >= 0 && first <= n_cells - n)) return 1;
  long long at = 0;
  for (long long i = 0; i < n; ++i) {
    const long long* c = cells + (size_t)(first + i) * POLY_CELL_WORDS;
    if (!(c[0] == at && c[1] > at && c[1] <= w)) return 1;
    at = c[1];
  }
  return at == w ? 2 : 1;
}

__global__ void __launch_bounds__(POLY_TILE_W * POLY_TILE_H)
k_poly_crop(const unsigned char* __restrict__ packed, long packed_bytes, const long long* __restrict__ regions, int R,
            const long long* __restrict__ cells, long n_cells, const int* __restrict__ tiles, unsigned char* __restrict__ out,
            long out_bytes) {
  const int* t = tiles + (size_t)blockIdx.x * 3;
  const int r = t[0], tile_row = t[1], tile_col = t[2];
  if (r < 0 || r >= R) return;
  const long long* p = regions + (size_t)r * POLY_REGION_WORDS;
  const int state = poly_region_state(p, cells, n_cells, packed_bytes, out_bytes);
  if (state == 0) return;
  const int H = (int)p[1], W = (int)p[2], h = (int)p[4], w = (int)p[5];
  // (the tile is data from the caller too: one outside its region writes nothing)
  if (tile_row < 0 || tile_col < 0 || tile_row > (h - 1) / POLY_TILE_H || tile_col > (w - 1) / POLY_TILE_W) return;
  const int x = tile_col * POLY_TILE_W + (int)threadIdx.x, y = tile_row * POLY_TILE_H + (int)threadIdx.y;
  if (x >= w || y >= h) return;
  unsigned char* dst = out + p[3] + ((size_t)y * w + x) * 3;
  unsigned char px[3] = {0, 0, 0};
  if (state == 2) {
    // the bounds ascend from 0 to w (poly_region_state) and x < w: the first cell whose x1 lies above x holds the pixel
    const long long* c = cells + (size_t)p[6] * POLY_CELL_WORDS;
    const int n = (int)p[7];
    int i = 0;
    while (i < n - 1 && (long long)x >= c[1]) {
      ++i;
      c += POLY_CELL_WORDS;
    }
    const double a0 = __longlong_as_double(c[2]), a1 = __longlong_as_double(c[3]), a2 = __longlong_as_double(c[4]);
    const double a3 = __longlong_as_double(c[5]), a4 = __longlong_as_double(c[6]), a5 = __longlong_as_double(c[7]);
    const double a6 = __longlong_as_double(c[8]), a7 = __longlong_as_double(c[9]);
    const double xin = (double)(x - (int)c[0]) + 0.5, yin = y + 0.5;
    const double sx = a0 + a1 * xin + a2 * yin + a3 * xin * yin;
    const double sy = a4 + a5 * xin + a6 * yin + a7 * xin * yin;
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

int dpmn_poly_crop_u8(const unsigned char* packed, long packed_bytes, const long long* regions, const long long* regions_host, int R,
                      const long long* cells, const long long* cells_host, int n_cells, const int* tiles, int n_tiles, unsigned char* out,
                      long out_bytes, dpmn_stream_t stream) {
  if (R == 0) return DPMN_OK;
  DPMN_REQUIRE(packed && regions && regions_host && cells && cells_host && out, "poly_crop: null pointer");
  DPMN_REQUIRE(R > 0 && n_cells > 0 && n_tiles >= 0 && (tiles || n_tiles == 0), "poly_crop: bad sizes");
  DPMN_REQUIRE(packed_bytes > 0 && out_bytes > 0, "poly_crop: empty buffers");
  int bad = 0;
  for (int r = 0; r < R; ++r)
    bad += poly_region_state(regions_host + (size_t)r * POLY_REGION_WORDS, cells_host, n_cells, packed_bytes, out_bytes) != 2;
  if (n_tiles > 0) {
    hipLaunchKernelGGL(k_poly_crop, dim3((unsigned)n_tiles), dim3(POLY_TILE_W, POLY_TILE_H), 0, as_stream(stream), packed, packed_bytes, regions,
                       R, cells, (long)n_cells, tiles, out, out_bytes);
    DPMN_CHECK_LAUNCH();
  }
  // the launch has gone out: the sound regions are computed, the others are black
  DPMN_REQUIRE(bad == 0, "poly_crop: a region does not fit the buffers, has a side outside 1 .. 8192 or cells that do not ascend from 0 "
                         "to its width inside the cell table (it is not read and comes out black)");
  return DPMN_OK;
}

}  // extern "C"
