// HR text crops from strings (main.py --train_words): B words laid out of a glyph atlas into a RAGGED batch of RGB uint8 images, packed
// back to back in the layout of utils/resize.py pack_ragged, in ONE launch.  The semantics are those of utils/render.py render_u8 (the
// CPU reference; its docstring states every formula), integers only, so every byte is reproduced:
//   scaled advances and pen positions of the string -> undo the shear -> the glyph under the pixel -> integer bilinear sample of its
//   alpha cell (Q16, round half up) -> background (flat or a linear gradient, + grain from the counter hash of degrade.hip) -> blend
// One block = one 8 x 128 tile of one image (host-built tile table, as degrade.hip), a lane = 4 neighbouring pixels of a row.  The block
// stages the string's cells, advances and pen positions in LDS once and finds the glyph under the tile's leftmost text column once; a
// pixel walks on from there (the text column grows with x), never from column 0.  A lane stores its 12 bytes as three dwords where the
// row's first byte is dword-aligned in memory, byte by byte otherwise and for the last w % 4 pixels of a row.
// Launch- and latency-bound work on a few hundred KB per batch.
#include "u8_pixel.h"

namespace {

constexpr int RD_THREADS = 256;
constexpr int RD_TILE_H = 8, RD_TILE_W = 128;      // RD_THREADS lanes x 4 pixels
constexpr int RD_MAX_LEN = 25;
constexpr int RD_N_GLYPH = 37;
constexpr int RD_PARAMS = 24;
// columns of a params row (utils/render.py)
constexpr int P_FONT = 0, P_CASE = 1, P_GH = 2, P_SPACING = 3, P_LEFT = 4, P_TOP = 6, P_SHEAR = 8, P_FG = 9, P_BG = 12, P_STYLE = 15,
              P_BG2 = 16, P_SEED = 19;

// atlas coordinate of the scaled index i along one axis: pixel centres, Q16, clamped to [0, limit]
__device__ __forceinline__ void axis_sample(int i, long long sc, int limit, int& i0, int& i1, long long& frac) {
  long long q = (((2ll * i + 1) * sc) >> 1) - 32768;
  if (q < 0) q = 0;
  i0 = min((int)(q >> 16), limit);
  i1 = min(i0 + 1, limit);
  frac = q & 0xFFFF;
}

__device__ __forceinline__ int grain_at(unsigned long long seed, unsigned long long pixel) {
  unsigned long long z = (pixel * 4ull) * DROP_PHI + seed;
  z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
  z ^= z >> 27; z *= 0x94D049BB133111EBull;
  z ^= z >> 31;
  return (int)((z >> 40) % 9ull) - 4;
}

__global__ void __launch_bounds__(RD_THREADS)
k_render_words(const int* __restrict__ classes, const int* __restrict__ lengths, const long long* __restrict__ params,
               const unsigned char* __restrict__ atlas, const int* __restrict__ advance, const int* __restrict__ atlas_h,
               const long long* __restrict__ items, const int* __restrict__ tiles, int n_tiles, unsigned char* __restrict__ out,
               long out_bytes, int B, int n_fonts, int GH, int GW) {
  __shared__ int s_pen[RD_MAX_LEN + 1], s_adv[RD_MAX_LEN], s_cellw[RD_MAX_LEN];
  __shared__ long s_cell[RD_MAX_LEN];
  __shared__ int s_first;
  const int tile = blockIdx.x;
  if (tile >= n_tiles) return;
  const int b = tiles[tile * 3], ty = tiles[tile * 3 + 1], tx = tiles[tile * 3 + 2];
  if (b < 0 || b >= B || ty < 0 || tx < 0) return;
  // ---- the image: numbers from the caller, so an image or a tile that does not fit the buffer is not written
  const long long* it = items + (size_t)b * 4;
  const long long off = it[0], h64 = it[1], w64 = it[2];
  if (h64 < 1 || h64 > RESIZE_MAX_SIDE || w64 < 1 || w64 > RESIZE_MAX_SIDE || off < 0 || off > out_bytes - h64 * w64 * 3) return;
  const int h = (int)h64, w = (int)w64;
  const int ty0 = ty * RD_TILE_H, tx0 = tx * RD_TILE_W;
  if (ty0 >= h || tx0 >= w) return;
  const long long* P = params + (size_t)b * RD_PARAMS;
  const int f = min(max((int)P[P_FONT], 0), n_fonts - 1), cs = (int)P[P_CASE], gh = max((int)P[P_GH], 1), sp = (int)P[P_SPACING];
  const int left = (int)P[P_LEFT], top = (int)P[P_TOP], s = (int)P[P_SHEAR], style = (int)P[P_STYLE];
  const int A = min(max(atlas_h[f], 1), GH);
  const int n = min(max(lengths[b], 1), RD_MAX_LEN);
  const int room = (int)(((long long)abs(s) * gh + 65535) >> 16);
  const int x0 = left + (s < 0 ? room : 0), base = top + gh - 1;

  // ---- the string, once per block: cells, scaled advances, pen positions, the glyph under the tile's leftmost text column
  if (threadIdx.x < n) {
    const int k = threadIdx.x;
    const int c = min(max(classes[b * RD_MAX_LEN + k], 0), RD_N_GLYPH - 1);
    const int plane = (cs == 1 || (cs == 2 && k == 0)) ? 1 : 0;
    const int cell = (f * 2 + plane) * RD_N_GLYPH + c;
    const int adv = min(max(advance[cell], 1), GW);
    s_cell[k] = (long)cell * GH * GW;
    s_cellw[k] = adv;
    s_adv[k] = max(1, (int)(((long long)adv * gh + A / 2) / A));
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int pen = 0;
    for (int k = 0; k < n; ++k) { s_pen[k] = pen; pen += max(s_adv[k] + sp, 0); }
    s_pen[n] = pen;
    // the smallest text column of the tile: its first pixel column under the largest shift of its rows (the shift is monotonic in y)
    const int y_last = min(ty0 + RD_TILE_H, h) - 1;
    const int shift = max((s * (base - ty0)) >> 16, (s * (base - y_last)) >> 16);
    const int u_min = tx0 - shift - x0;
    int k = 0;
    while (k + 1 < n && u_min >= s_pen[k + 1]) ++k;
    s_first = k;
  }
  __syncthreads();

  const int y = ty0 + (int)(threadIdx.x >> 5), x = tx0 + (int)(threadIdx.x & 31) * 4;
  if (y >= h || x >= w) return;
  const int npx = min(4, w - x);
  const int tw = max(s_pen[n] - sp, 1);
  const int v = y - top, u_row = x - ((s * (base - y)) >> 16) - x0;
  const long long sc = ((long long)A << 16) / gh;
  const unsigned long long seed = (unsigned long long)P[P_SEED];
  int fg[3], bg[3], bg2[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    fg[c] = min(max((int)P[P_FG + c], 0), 255);
    bg[c] = min(max((int)P[P_BG + c], 0), 255);
    bg2[c] = min(max((int)P[P_BG2 + c], 0), 255);
  }
  int y_0 = 0, y_1 = 0;
  long long fy = 0;
  const bool row_in = v >= 0 && v < gh;
  if (row_in) axis_sample(v, sc, A - 1, y_0, y_1, fy);

  unsigned int word[3] = {0u, 0u, 0u};      // the lane's 12 bytes, little endian
  int k = s_first;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (i >= npx) break;
    const int u = u_row + i;
    int alpha = 0;
    if (row_in && u >= 0 && u < tw) {
      while (k + 1 < n && u >= s_pen[k + 1]) ++k;
      const int ug = u - s_pen[k];
      if (ug >= 0 && ug < s_adv[k]) {
        int x_0, x_1;
        long long fx;
        axis_sample(ug, sc, s_cellw[k] - 1, x_0, x_1, fx);
        const unsigned char* cell = atlas + s_cell[k];
        const long long a00 = cell[y_0 * GW + x_0], a01 = cell[y_0 * GW + x_1], a10 = cell[y_1 * GW + x_0], a11 = cell[y_1 * GW + x_1];
        const unsigned long long t = (unsigned long long)(a00 * (65536 - fx) + a01 * fx), bt = (unsigned long long)(a10 * (65536 - fx) + a11 * fx);
        alpha = (int)((t * (unsigned long long)(65536 - fy) + bt * (unsigned long long)fy + (1ull << 31)) >> 32);
      }
    }
    const int g = grain_at(seed, (unsigned long long)y * (unsigned long long)w + (unsigned long long)(x + i));
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      int back = bg[c];
      if (style == 1) {
        const int m = max(w - 1, 1);
        back = (bg[c] * (m - (x + i)) + bg2[c] * (x + i) + m / 2) / m;
      } else if (style == 2) {
        const int m = max(h - 1, 1);
        back = (bg[c] * (m - y) + bg2[c] * y + m / 2) / m;
      }
      back = min(max(back + g, 0), 255);
      const unsigned int val = (unsigned int)((fg[c] * alpha + back * (255 - alpha) + 127) / 255);
      const int byte = i * 3 + c;
      word[byte >> 2] |= val << ((byte & 3) * 8);
    }
  }
  unsigned char* dst = out + off + ((size_t)y * w + x) * 3;
  if (npx == 4 && ((size_t)dst & 3) == 0) {
    unsigned int* d4 = reinterpret_cast<unsigned int*>(dst);
    d4[0] = word[0]; d4[1] = word[1]; d4[2] = word[2];
  } else {
#pragma unroll
    for (int byte = 0; byte < 12; ++byte)
      if (byte < npx * 3) dst[byte] = (unsigned char)(word[byte >> 2] >> ((byte & 3) * 8));
  }
}

}  // namespace

extern "C" {

int dpmn_render_words_u8(const int* classes, const int* lengths, const long long* params, const unsigned char* atlas_u8, const int* advance,
                         const int* atlas_h, const long long* meta, const int* tiles, int n_tiles, unsigned char* out_packed, long out_bytes,
                         int B, int n_fonts, int GH, int GW, const int* host_classes, const int* host_lengths, const long long* host_params,
                         const long long* host_meta, dpmn_stream_t stream) {
  DPMN_REQUIRE(classes && lengths && params && atlas_u8 && advance && atlas_h && meta && tiles && out_packed, "render_words: null pointer");
  DPMN_REQUIRE(host_classes && host_lengths && host_params && host_meta, "render_words: the host copies of classes, lengths, params and meta are required (they are checked here)");
  DPMN_REQUIRE(B > 0 && B <= 65535, "render_words: bad batch size (1 <= B <= 65535)");
  DPMN_REQUIRE(n_fonts > 0 && GH > 0 && GH <= 256 && GW > 0 && GW <= 1024, "render_words: bad atlas (fonts >= 1, cell 1 .. 256 x 1 .. 1024)");
  DPMN_REQUIRE(n_tiles >= B && out_bytes > 0, "render_words: bad sizes (a tile per image at least)");
  long n_expected = 0;
  for (int b = 0; b < B; ++b) {
    DPMN_REQUIRE(host_lengths[b] >= 1 && host_lengths[b] <= RD_MAX_LEN, "render_words: a word's length is outside 1 .. 25");
    for (int k = 0; k < host_lengths[b]; ++k)
      DPMN_REQUIRE(host_classes[b * RD_MAX_LEN + k] >= 0 && host_classes[b * RD_MAX_LEN + k] < RD_N_GLYPH, "render_words: a class outside the atlas (0 .. 36)");
    const long long* P = host_params + (size_t)b * RD_PARAMS;
    DPMN_REQUIRE(P[P_FONT] >= 0 && P[P_FONT] < n_fonts, "render_words: a font index out of range");
    DPMN_REQUIRE(P[P_GH] >= 1 && P[P_GH] <= 256 && P[P_SHEAR] >= -65536 && P[P_SHEAR] <= 65536 && P[P_SPACING] >= -1 && P[P_SPACING] <= 64 &&
                 P[P_LEFT] >= 0 && P[P_LEFT] <= RESIZE_MAX_SIDE && P[P_TOP] >= 0 && P[P_TOP] <= RESIZE_MAX_SIDE,
                 "render_words: a params row is outside its domain");
    const long long off = host_meta[b * 4], h = host_meta[b * 4 + 1], w = host_meta[b * 4 + 2];
    DPMN_REQUIRE(h >= 1 && h <= RESIZE_MAX_SIDE && w >= 1 && w <= RESIZE_MAX_SIDE, "render_words: an image side outside 1 .. 8192");
    DPMN_REQUIRE(off >= 0 && off <= out_bytes - h * w * 3, "render_words: an image lies outside the output buffer");
    n_expected += ((h + RD_TILE_H - 1) / RD_TILE_H) * ((w + RD_TILE_W - 1) / RD_TILE_W);
  }
  DPMN_REQUIRE(n_expected == n_tiles, "render_words: the tile table does not cover the images (8 x 128 tiles)");
  hipLaunchKernelGGL(k_render_words, dim3((unsigned)n_tiles), dim3(RD_THREADS), 0, as_stream(stream), classes, lengths, params, atlas_u8,
                     advance, atlas_h, meta, tiles, n_tiles, out_packed, out_bytes, B, n_fonts, GH, GW);
  DPMN_CHECK_LAUNCH();
  return DPMN_OK;
}

}  // extern "C"
